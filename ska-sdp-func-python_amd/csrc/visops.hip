// Visibility operations for gfx950 (reference src/ska_sdp_func_python/
// visibility/operations.py):
//   sdp_hip_vis_average_channels   integrate_visibility_by_channel (:192-235)
//                                  and average_visibility_by_channel (:238-306)
//   sdp_hip_vis_to_stokes          convert_visibility_to_stokes (:309-333) and
//                                  convert_visibility_to_stokesI (:336-420)
//   sdp_hip_vis_remove_continuum   remove_continuum_visibility (:108-142)
//
// All visibility-shaped arrays are the Visibility's [ntimes, nbl, nchan, npol]
// in C order.  Arithmetic follows the reference's fp64 operations in numpy's
// order (visops_math.h); complex division is numpy's (Smith's algorithm); fp
// contraction is off.  The kernels are HBM-bound streaming passes: every
// array is read once, through loads in which adjacent lanes read adjacent
// elements, and the channel reductions run out of LDS in a fixed order, so
// no result depends on the launch geometry.
#include "sdp_common.h"
#include "visops_math.h"

#pragma clang fp contract(off)

namespace sdp {
namespace visops {

struct cplx {
    double re, im;
};

__device__ __forceinline__ cplx cmul(cplx a, cplx b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }

// numpy's complex division (umath loops: Smith's algorithm), as in calops.hip
__device__ __forceinline__ cplx cdiv(cplx a, cplx b) {
    const double abr = fabs(b.re), abi = fabs(b.im);
    if (abr >= abi) {
        if (abr == 0.0 && abi == 0.0) return {a.re / abr, a.im / abr};
        const double rat = b.im / b.re;
        const double scl = 1.0 / (b.re + b.im * rat);
        return {(a.re + a.im * rat) * scl, (a.im - a.re * rat) * scl};
    }
    const double rat = b.re / b.im;
    const double scl = 1.0 / (b.im + b.re * rat);
    return {(a.re * rat + a.im) * scl, (a.im * rat - a.re) * scl};
}

__device__ __forceinline__ cplx load_c(const void *p, int c128, size_t i) {
    if (c128) {
        const double2 v = static_cast<const double2 *>(p)[i];
        return {v.x, v.y};
    }
    const float2 v = static_cast<const float2 *>(p)[i];
    return {(double)v.x, (double)v.y};
}

__device__ __forceinline__ void store_c(void *p, int c128, size_t i, cplx v) {
    if (c128) static_cast<double2 *>(p)[i] = make_double2(v.re, v.im);
    else static_cast<float2 *>(p)[i] = make_float2((float)v.re, (float)v.im);
}

__device__ __forceinline__ int flag_of(const void *flags, int bytes, size_t i) {
    if (!bytes) return 0;
    if (bytes == 8) return (int)static_cast<const int64_t *>(flags)[i];
    if (bytes == 4) return (int)static_cast<const int32_t *>(flags)[i];
    return (int)static_cast<const int8_t *>(flags)[i];
}

__device__ __forceinline__ void store_flag(void *flags, int bytes, size_t i, int f) {
    if (bytes == 8) static_cast<int64_t *>(flags)[i] = f;
    else if (bytes == 4) static_cast<int32_t *>(flags)[i] = f;
    else static_cast<int8_t *>(flags)[i] = (int8_t)f;
}

// ---- channel averaging ------------------------------------------------------
// The input is a sequence of groups of G channels x npol elements, contiguous
// in memory (G divides nchan), and output element (group, pol) is a sum over
// the group's channels.  k_average_tiled stages kAvgTile consecutive elements
// (a whole number of groups, across row boundaries) per pass and one lane per
// output element adds its G channels from LDS; k_average_long serves groups
// larger than a tile, one workgroup per group.
constexpr int kAvgThreads = 256;
constexpr int kAvgTile = 512;                     // elements staged per pass
constexpr int kAvgLds = kAvgTile + kAvgTile / 8;  // with the padding of lds_at
constexpr int kAvgMaxBlocks = 4096;

// 4 doubles of padding after every 32: lanes of different groups that read the
// same channel of their group do not all fall on the same banks
__device__ __forceinline__ int lds_at(int i) { return i + ((i >> 5) << 2); }

struct AvgArgs {
    const void *vis;
    const double *weight, *iw;
    const void *flags;
    void *vis_out;
    double *w_out, *iw_out;
    void *fl_out;
    int64_t ngroups;
    int c128, fbytes, out_fbytes, variant, nchan, npol, G;
};

struct AvgTerm {
    cplx num;
    double fw, fiw;
    int fl;
};

// one sample's terms of the four sums.  variant 0 (integrate, :205-213):
// vis * flagged_weight; variant 1 (average, :282-289): flagged_vis * weight
__device__ __forceinline__ AvgTerm avg_term(const AvgArgs &a, size_t i) {
    AvgTerm t;
    t.fl = flag_of(a.flags, a.fbytes, i);
    const double keep = 1.0 - (double)t.fl;
    const cplx v = load_c(a.vis, a.c128, i);
    const double w = a.weight[i];
    t.fw = w * keep;
    t.fiw = a.iw[i] * keep;
    t.num = a.variant == 0 ? cmul(v, {t.fw, 0.0}) : cmul(cmul(v, {keep, 0.0}), {w, 0.0});
    return t;
}

// the flag rule (:201-203, :291-293: the count is compared with the total
// nchan in both functions) and the division where the kept weight is positive
__device__ __forceinline__ void avg_finish(const AvgArgs &a, size_t o, cplx num, double sw,
                                           double siw, int sfl) {
    int f = sfl;
    if (f < a.nchan) f = 0;
    if (f > 1) f = 1;
    const double d = sw * (double)(1 - f);
    if (d > 0.0) num = cdiv(num, {d, 0.0});
    store_c(a.vis_out, a.c128, o, num);
    a.w_out[o] = sw;
    a.iw_out[o] = siw;
    store_flag(a.fl_out, a.out_fbytes, o, f);
}

// PAIRWISE: npol == 1, numpy's pairwise order (visops_math.h)
template <bool PAIRWISE>
__global__ __launch_bounds__(kAvgThreads) void k_average_tiled(AvgArgs a, int groups_per_tile) {
    __shared__ double s_re[kAvgLds], s_im[kAvgLds], s_fw[kAvgLds], s_fiw[kAvgLds];
    __shared__ int s_fl[kAvgLds];
    const int ge = a.G * a.npol;  // elements per group
    const int64_t ntiles = (a.ngroups + groups_per_tile - 1) / groups_per_tile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t g0 = tile * groups_per_tile;
        const int ng = (int)imin64(groups_per_tile, a.ngroups - g0);
        const int n = ng * ge;
        const size_t e0 = (size_t)g0 * ge;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kAvgThreads) {
            const AvgTerm t = avg_term(a, e0 + i);
            const int l = lds_at(i);
            s_re[l] = t.num.re;
            s_im[l] = t.num.im;
            s_fw[l] = t.fw;
            s_fiw[l] = t.fiw;
            s_fl[l] = t.fl;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < ng * a.npol; j += kAvgThreads) {
            const int base = (j / a.npol) * ge + j % a.npol;
            cplx num = {0.0, 0.0};
            double sw = 0.0, siw = 0.0;
            int sfl = 0;
            if (PAIRWISE) {
                num.re = numpy_sum<4>([&](int64_t c) { return s_re[lds_at((int)c)]; }, base, a.G);
                num.im = numpy_sum<4>([&](int64_t c) { return s_im[lds_at((int)c)]; }, base, a.G);
                sw = numpy_sum<8>([&](int64_t c) { return s_fw[lds_at((int)c)]; }, base, a.G);
                siw = numpy_sum<8>([&](int64_t c) { return s_fiw[lds_at((int)c)]; }, base, a.G);
                for (int c = 0; c < a.G; ++c) sfl += s_fl[lds_at(base + c)];
            } else {
                for (int c = 0; c < a.G; ++c) {
                    const int l = lds_at(base + c * a.npol);
                    num = cadd(num, {s_re[l], s_im[l]});
                    sw += s_fw[l];
                    siw += s_fiw[l];
                    sfl += s_fl[l];
                }
            }
            avg_finish(a, (size_t)g0 * a.npol + j, num, sw, siw, sfl);
        }
    }
}

// groups of more than kAvgTile elements.  npol 2 and 4: lanes 0..npol-1 carry
// their sums from tile to tile, channel by channel.  npol 1: numpy's pairwise
// order is a tree over the whole group, which three lanes walk in global
// memory (complex sum; weight and flags; imaging weight).
template <bool PAIRWISE>
__global__ __launch_bounds__(kAvgThreads) void k_average_long(AvgArgs a) {
    __shared__ double s_re[kAvgLds], s_im[kAvgLds], s_fw[kAvgLds], s_fiw[kAvgLds];
    __shared__ int s_fl[kAvgLds];
    const int ge = a.G * a.npol;
    for (int64_t g = blockIdx.x; g < a.ngroups; g += gridDim.x) {
        const size_t e0 = (size_t)g * ge;
        if (PAIRWISE) {
            __syncthreads();
            if (threadIdx.x == 0) {
                s_re[0] = numpy_sum<4>([&](int64_t c) { return avg_term(a, (size_t)c).num.re; }, (int64_t)e0, a.G);
                s_im[0] = numpy_sum<4>([&](int64_t c) { return avg_term(a, (size_t)c).num.im; }, (int64_t)e0, a.G);
            } else if (threadIdx.x == 1) {
                s_fw[0] = numpy_sum<8>([&](int64_t c) { return avg_term(a, (size_t)c).fw; }, (int64_t)e0, a.G);
                int sfl = 0;
                for (int c = 0; c < a.G; ++c) sfl += flag_of(a.flags, a.fbytes, e0 + c);
                s_fl[0] = sfl;
            } else if (threadIdx.x == 2) {
                s_fiw[0] = numpy_sum<8>([&](int64_t c) { return avg_term(a, (size_t)c).fiw; }, (int64_t)e0, a.G);
            }
            __syncthreads();
            if (threadIdx.x == 0) avg_finish(a, (size_t)g, {s_re[0], s_im[0]}, s_fw[0], s_fiw[0], s_fl[0]);
            continue;
        }
        cplx num = {0.0, 0.0};
        double sw = 0.0, siw = 0.0;
        int sfl = 0;
        for (int t0 = 0; t0 < ge; t0 += kAvgTile) {
            const int n = min(kAvgTile, ge - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += kAvgThreads) {
                const AvgTerm t = avg_term(a, e0 + t0 + i);
                const int l = lds_at(i);
                s_re[l] = t.num.re;
                s_im[l] = t.num.im;
                s_fw[l] = t.fw;
                s_fiw[l] = t.fiw;
                s_fl[l] = t.fl;
            }
            __syncthreads();
            if ((int)threadIdx.x < a.npol) {
                for (int i = threadIdx.x; i < n; i += a.npol) {
                    const int l = lds_at(i);
                    num = cadd(num, {s_re[l], s_im[l]});
                    sw += s_fw[l];
                    siw += s_fiw[l];
                    sfl += s_fl[l];
                }
            }
        }
        if ((int)threadIdx.x < a.npol) avg_finish(a, (size_t)g * a.npol + threadIdx.x, num, sw, siw, sfl);
    }
}

// ---- Stokes conversion ------------------------------------------------------
constexpr int kStokesThreads = 256;
constexpr int kStokesMaxBlocks = 4096;

struct StokesMatrix {
    double re[16], im[16];  // [output pol][input pol]
};

// convert_visibility_to_stokes: vis <- M vis per sample, every pol's flag <-
// flag[0] | flag[3], in place
__global__ __launch_bounds__(kStokesThreads) void k_to_stokes_iquv(int64_t nsamp, void *vis,
                                                                   int c128, void *flags,
                                                                   int fbytes, StokesMatrix m) {
    for (int64_t s = blockIdx.x * (int64_t)kStokesThreads + threadIdx.x; s < nsamp;
         s += (int64_t)gridDim.x * kStokesThreads) {
        const size_t b = (size_t)s * 4;
        cplx v[4];
        for (int p = 0; p < 4; ++p) v[p] = load_c(vis, c128, b + p);
        for (int o = 0; o < 4; ++o) {
            cplx acc = cmul({m.re[o * 4], m.im[o * 4]}, v[0]);
            for (int p = 1; p < 4; ++p) acc = cadd(acc, cmul({m.re[o * 4 + p], m.im[o * 4 + p]}, v[p]));
            store_c(vis, c128, b + o, acc);
        }
        if (fbytes) {
            const int f = (flag_of(flags, fbytes, b) != 0 || flag_of(flags, fbytes, b + 3) != 0) ? 1 : 0;
            for (int p = 0; p < 4; ++p) store_flag(flags, fbytes, b + p, f);
        }
    }
}

// convert_visibility_to_stokesI: half the sum of the two parallel hands of
// the flagged visibilities, their flagged weights summed, the flags or-ed
__global__ __launch_bounds__(kStokesThreads) void k_to_stokes_i(
    int64_t nsamp, int npol, const void *__restrict__ vis, int c128,
    const double *__restrict__ weight, const double *__restrict__ iw,
    const void *__restrict__ flags, int fbytes, void *vis_out, double *w_out, double *iw_out,
    void *fl_out, int out_fbytes) {
    for (int64_t s = blockIdx.x * (int64_t)kStokesThreads + threadIdx.x; s < nsamp;
         s += (int64_t)gridDim.x * kStokesThreads) {
        const size_t i0 = (size_t)s * npol, i1 = i0 + npol - 1;
        const int f0 = flag_of(flags, fbytes, i0), f1 = flag_of(flags, fbytes, i1);
        const double k0 = 1.0 - (double)f0, k1 = 1.0 - (double)f1;
        const cplx a = cmul(load_c(vis, c128, i0), {k0, 0.0});
        const cplx b = cmul(load_c(vis, c128, i1), {k1, 0.0});
        store_c(vis_out, c128, (size_t)s, cmul({0.5, 0.0}, cadd(a, b)));
        w_out[s] = weight[i0] * k0 + weight[i1] * k1;
        iw_out[s] = iw[i0] * k0 + iw[i1] * k1;
        store_flag(fl_out, out_fbytes, (size_t)s, (f0 != 0 || f1 != 0) ? 1 : 0);
    }
}

// ---- continuum removal ------------------------------------------------------
// One spectrum is one (row, pol) (fit_subtract, visops_math.h).
// k_continuum_lds: a workgroup loads `rows` consecutive rows, contiguous in
// memory, into LDS with coalesced loads; `lanes` adjacent lanes (a power of
// two, chosen from nchan and npol alone) share a spectrum, each taking every
// lanes-th channel, their partial sums combined by a butterfly of
// cross-lane reads; the block is written back coalesced.  k_continuum_global
// serves rows too long for LDS straight from global memory, one lane each.
constexpr int kContThreads = 256;
constexpr int kContMaxBlocks = 1024;
constexpr int kContLdsTarget = 40 * 1024;  // per workgroup: four workgroups share a CU's 160 KiB
constexpr int kContLdsLimit = 60 * 1024;   // a single row above this goes to k_continuum_global
constexpr int kContRowPad = 4;             // doubles between rows in LDS (bank spread)

struct ContArgs {
    void *vis;
    const double *weight;
    const void *flags;
    const double *x;
    const uint8_t *mask;
    int32_t *rank_list, *rank_count;
    int64_t nrows;
    int c128, fbytes, nchan, npol, rank_capacity;
};

// the fit weight: flagged_weight, 0 where mask is True (:132-136)
__device__ __forceinline__ double fit_weight(const ContArgs &a, size_t i, int c) {
    const double keep = 1.0 - (double)flag_of(a.flags, a.fbytes, i);
    const double w = a.weight[i] * keep;
    return (a.mask && a.mask[c]) ? 0.0 : w;
}

__device__ __forceinline__ void note_deficient(const ContArgs &a, int64_t spectrum) {
    const int slot = atomicAdd(a.rank_count, 1);
    if (slot < a.rank_capacity) a.rank_list[slot] = (int32_t)spectrum;
}

struct LdsSpectrum {
    const double *sx;
    double *re, *im;
    const double *sw;
    int npol, lane, lanes;
    __device__ int first() const { return lane; }
    __device__ int step() const { return lanes; }
    __device__ double sum(double v) const {
        for (int m = 1; m < lanes; m <<= 1) v += __shfl_xor(v, m);
        return v;
    }
    __device__ double x(int c) const { return sx[c]; }
    __device__ double w(int c) const { return sw[c * npol]; }
    __device__ double yre(int c) const { return re[c * npol]; }
    __device__ double yim(int c) const { return im[c * npol]; }
    __device__ void sub(int c, double fr, double fi) {
        re[c * npol] -= fr;
        im[c * npol] -= fi;
    }
};

template <int DEG>
__global__ __launch_bounds__(kContThreads) void k_continuum_lds(ContArgs a, int rows, int rowstride,
                                                                int lanes) {
    extern __shared__ double sm[];
    double *sx = sm;
    double *s_re = sx + a.nchan;
    double *s_im = s_re + (size_t)rows * rowstride;
    double *s_w = s_im + (size_t)rows * rowstride;
    const int E = a.nchan * a.npol;
    for (int c = threadIdx.x; c < a.nchan; c += kContThreads) sx[c] = a.x[c];
    const int64_t nchunks = (a.nrows + rows - 1) / rows;
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int64_t row0 = ch * rows;
        const int nr = (int)imin64(rows, a.nrows - row0);
        const int n = nr * E;
        const size_t e0 = (size_t)row0 * E;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kContThreads) {
            const int r = i / E, e = i - r * E;
            const cplx v = load_c(a.vis, a.c128, e0 + i);
            const int l = r * rowstride + e;
            s_re[l] = v.re;
            s_im[l] = v.im;
            s_w[l] = fit_weight(a, e0 + i, e / a.npol);
        }
        __syncthreads();
        if ((int)threadIdx.x < nr * a.npol * lanes) {
            const int s = threadIdx.x / lanes, q = threadIdx.x % lanes;
            const int r = s / a.npol, p = s % a.npol;
            const int l = r * rowstride + p;
            LdsSpectrum sp{sx, s_re + l, s_im + l, s_w + l, a.npol, q, lanes};
            if (fit_subtract<DEG>(sp, a.nchan) == kFitDeficient && q == 0)
                note_deficient(a, (row0 + r) * a.npol + p);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kContThreads) {
            const int r = i / E, e = i - r * E;
            const int l = r * rowstride + e;
            store_c(a.vis, a.c128, e0 + i, {s_re[l], s_im[l]});
        }
    }
}

struct GlobalSpectrum {
    const ContArgs &a;
    size_t base;  // element of channel 0
    __device__ size_t at(int c) const { return base + (size_t)c * a.npol; }
    __device__ int first() const { return 0; }
    __device__ int step() const { return 1; }
    __device__ double sum(double v) const { return v; }
    __device__ double x(int c) const { return a.x[c]; }
    __device__ double w(int c) const { return fit_weight(a, at(c), c); }
    __device__ double yre(int c) const { return load_c(a.vis, a.c128, at(c)).re; }
    __device__ double yim(int c) const { return load_c(a.vis, a.c128, at(c)).im; }
    __device__ void sub(int c, double fr, double fi) {
        const cplx v = load_c(a.vis, a.c128, at(c));
        store_c(a.vis, a.c128, at(c), {v.re - fr, v.im - fi});
    }
};

template <int DEG>
__global__ __launch_bounds__(kContThreads) void k_continuum_global(ContArgs a) {
    const int64_t nspec = a.nrows * a.npol;
    for (int64_t s = blockIdx.x * (int64_t)kContThreads + threadIdx.x; s < nspec;
         s += (int64_t)gridDim.x * kContThreads) {
        const int64_t row = s / a.npol;
        const int p = (int)(s % a.npol);
        GlobalSpectrum sp{a, (size_t)row * a.nchan * a.npol + p};
        if (fit_subtract<DEG>(sp, a.nchan) == kFitDeficient) note_deficient(a, s);
    }
}

template <int DEG>
void launch_continuum(const ContArgs &a, hipStream_t st) {
    const size_t row_doubles = (size_t)a.nchan * a.npol + kContRowPad;
    const size_t fixed = (size_t)a.nchan * sizeof(double);
    const size_t per_row = row_doubles * 3 * sizeof(double);
    if (fixed + per_row > (size_t)kContLdsLimit) {
        const int64_t nspec = a.nrows * a.npol;
        const unsigned nb = (unsigned)std::min<int64_t>((nspec + kContThreads - 1) / kContThreads,
                                                       kContMaxBlocks);
        k_continuum_global<DEG><<<nb, kContThreads, 0, st>>>(a);
        return;
    }
    int rows = (int)(((size_t)kContLdsTarget - std::min(fixed, (size_t)kContLdsTarget)) / per_row);
    rows = std::max(1, std::min(rows, kContThreads / a.npol));
    // lanes per spectrum: as many as the workgroup has for its spectra, within
    // a wave, and no more than there are channels
    int lanes = 1;
    while (lanes * 2 <= 64 && lanes * 2 <= a.nchan && rows * a.npol * lanes * 2 <= kContThreads)
        lanes *= 2;
    const size_t bytes = fixed + (size_t)rows * per_row;
    const int64_t nchunks = (a.nrows + rows - 1) / rows;
    const unsigned nb = (unsigned)std::min<int64_t>(nchunks, kContMaxBlocks);
    k_continuum_lds<DEG><<<nb, kContThreads, bytes, st>>>(a, rows, (int)row_doubles, lanes);
}

void check_common(int64_t nrows, int nchan, int npol, int vis_dtype, const void *flags,
                  int flag_bytes) {
    SDP_REQUIRE(nrows >= 0 && nchan > 0, "bad visibility dimensions");
    SDP_REQUIRE(npol == 1 || npol == 2 || npol == 4, "npol must be 1, 2 or 4");
    SDP_REQUIRE(vis_dtype == SDP_HIP_C64 || vis_dtype == SDP_HIP_C128,
                "visibilities must be complex64 or complex128");
    SDP_REQUIRE(!flags || flag_bytes == 1 || flag_bytes == 4 || flag_bytes == 8,
                "flag element size must be 1, 4 or 8 bytes");
}

}  // namespace visops
}  // namespace sdp

extern "C" {

int sdp_hip_vis_average_channels(int64_t nrows, int nchan, int npol, int group, int variant,
                                 const void *vis, int vis_dtype, const double *weight,
                                 const double *imaging_weight, const void *flags, int flag_bytes,
                                 void *vis_out, double *weight_out, double *imaging_weight_out,
                                 void *flags_out, int flags_out_bytes, void *stream, char *errbuf,
                                 size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::visops;
    return guarded(errbuf, errbuf_len, [&] {
        check_common(nrows, nchan, npol, vis_dtype, flags, flag_bytes);
        SDP_REQUIRE(group >= 1 && nchan % group == 0, "the group size must divide nchan");
        SDP_REQUIRE(variant == 0 || variant == 1, "variant must be 0 (integrate) or 1 (average)");
        SDP_REQUIRE(flags_out_bytes == 1 || flags_out_bytes == 4 || flags_out_bytes == 8,
                    "flag element size must be 1, 4 or 8 bytes");
        SDP_REQUIRE((int64_t)nchan * npol < ((int64_t)1 << 30), "nchan * npol must be below 2^30");
        if (nrows == 0) return;
        SDP_REQUIRE(vis && weight && imaging_weight && vis_out && weight_out &&
                        imaging_weight_out && flags_out,
                    "null pointer argument");
        AvgArgs a;
        a.vis = vis;
        a.weight = weight;
        a.iw = imaging_weight;
        a.flags = flags;
        a.vis_out = vis_out;
        a.w_out = weight_out;
        a.iw_out = imaging_weight_out;
        a.fl_out = flags_out;
        a.ngroups = nrows * (nchan / group);
        a.c128 = vis_dtype == SDP_HIP_C128;
        a.fbytes = flags ? flag_bytes : 0;
        a.out_fbytes = flags_out_bytes;
        a.variant = variant;
        a.nchan = nchan;
        a.npol = npol;
        a.G = group;
        const int ge = group * npol;
        if (ge <= kAvgTile) {
            const int gpt = kAvgTile / ge;
            const int64_t ntiles = (a.ngroups + gpt - 1) / gpt;
            const unsigned nb = (unsigned)std::min<int64_t>(ntiles, kAvgMaxBlocks);
            if (npol == 1) k_average_tiled<true><<<nb, kAvgThreads, 0, as_stream(stream)>>>(a, gpt);
            else k_average_tiled<false><<<nb, kAvgThreads, 0, as_stream(stream)>>>(a, gpt);
        } else {
            const unsigned nb = (unsigned)std::min<int64_t>(a.ngroups, kAvgMaxBlocks);
            if (npol == 1) k_average_long<true><<<nb, kAvgThreads, 0, as_stream(stream)>>>(a);
            else k_average_long<false><<<nb, kAvgThreads, 0, as_stream(stream)>>>(a);
        }
        SDP_HIP_CHECK(hipGetLastError());
    });
}

int sdp_hip_vis_to_stokes(int64_t nsamples, int npol, int mode, void *vis, int vis_dtype,
                          const double *weight, const double *imaging_weight, void *flags,
                          int flag_bytes, const double *matrix, void *vis_out, double *weight_out,
                          double *imaging_weight_out, void *flags_out, int flags_out_bytes,
                          void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::visops;
    return guarded(errbuf, errbuf_len, [&] {
        check_common(nsamples, 1, npol, vis_dtype, flags, flag_bytes);
        SDP_REQUIRE(mode == SDP_HIP_STOKES_IQUV || mode == SDP_HIP_STOKES_I,
                    "mode must be SDP_HIP_STOKES_IQUV or SDP_HIP_STOKES_I");
        if (mode == SDP_HIP_STOKES_IQUV) SDP_REQUIRE(npol == 4, "stokesIQUV needs 4 polarisations");
        else SDP_REQUIRE(npol == 2 || npol == 4, "stokesI needs 2 or 4 polarisations");
        if (nsamples == 0) return;
        const unsigned nb = (unsigned)std::min<int64_t>(
            (nsamples + kStokesThreads - 1) / kStokesThreads, kStokesMaxBlocks);
        if (mode == SDP_HIP_STOKES_IQUV) {
            SDP_REQUIRE(vis && matrix, "null pointer argument");
            StokesMatrix m;
            for (int k = 0; k < 16; ++k) {
                m.re[k] = matrix[2 * k];
                m.im[k] = matrix[2 * k + 1];
            }
            k_to_stokes_iquv<<<nb, kStokesThreads, 0, as_stream(stream)>>>(
                nsamples, vis, vis_dtype == SDP_HIP_C128, flags, flags ? flag_bytes : 0, m);
        } else {
            SDP_REQUIRE(vis && weight && imaging_weight && vis_out && weight_out &&
                            imaging_weight_out && flags_out,
                        "null pointer argument");
            SDP_REQUIRE(flags_out_bytes == 1 || flags_out_bytes == 4 || flags_out_bytes == 8,
                        "flag element size must be 1, 4 or 8 bytes");
            k_to_stokes_i<<<nb, kStokesThreads, 0, as_stream(stream)>>>(
                nsamples, npol, vis, vis_dtype == SDP_HIP_C128, weight, imaging_weight, flags,
                flags ? flag_bytes : 0, vis_out, weight_out, imaging_weight_out, flags_out,
                flags_out_bytes);
        }
        SDP_HIP_CHECK(hipGetLastError());
    });
}

int sdp_hip_vis_remove_continuum(int64_t nrows, int nchan, int npol, void *vis, int vis_dtype,
                                 const double *weight, const void *flags, int flag_bytes,
                                 const double *x, const uint8_t *mask, int degree,
                                 int32_t *rank_list, int rank_capacity, int32_t *rank_count,
                                 void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::visops;
    return guarded(errbuf, errbuf_len, [&] {
        check_common(nrows, nchan, npol, vis_dtype, flags, flag_bytes);
        SDP_REQUIRE(degree >= 0 && degree <= kMaxDegree,
                    "the polynomial degree must be between 0 and 5");
        SDP_REQUIRE(nchan >= 2, "remove_continuum needs at least 2 channels");
        SDP_REQUIRE(nrows * npol < ((int64_t)1 << 31), "more than 2^31 - 1 spectra");
        SDP_REQUIRE((int64_t)nchan * npol < ((int64_t)1 << 30), "nchan * npol must be below 2^30");
        SDP_REQUIRE(rank_count && rank_capacity >= 0 && (rank_list || rank_capacity == 0),
                    "the rank-deficient list needs its count and storage");
        const hipStream_t st = as_stream(stream);
        SDP_HIP_CHECK(hipMemsetAsync(rank_count, 0, sizeof(int32_t), st));
        if (nrows == 0) return;
        SDP_REQUIRE(vis && weight && x, "null pointer argument");
        ContArgs a;
        a.vis = vis;
        a.weight = weight;
        a.flags = flags;
        a.x = x;
        a.mask = mask;
        a.rank_list = rank_list;
        a.rank_count = rank_count;
        a.nrows = nrows;
        a.c128 = vis_dtype == SDP_HIP_C128;
        a.fbytes = flags ? flag_bytes : 0;
        a.nchan = nchan;
        a.npol = npol;
        a.rank_capacity = rank_capacity;
        switch (degree) {
            case 0: launch_continuum<0>(a, st); break;
            case 1: launch_continuum<1>(a, st); break;
            case 2: launch_continuum<2>(a, st); break;
            case 3: launch_continuum<3>(a, st); break;
            case 4: launch_continuum<4>(a, st); break;
            default: launch_continuum<5>(a, st); break;
        }
        SDP_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
