// w-stacking NUFFT, stage 1 (device): bounds and single-level bucketing.
//   k_bounds / k_bounds_final   fp64 w range and uv extent of the rows
//   VisExtra, eff_weight, eff_vis, conv_vis, t_load
//                               typed loads of weights, flags and visibilities
//                               (pol conversion included), shared with the
//                               two-level passes (k_t_*)
//   dispatch_int                runtime value to template argument
//   k_bucket                    count pass (kScatter = false) and value pass
//                               (true) of the single-level histogram: one-cell
//                               keys (g.sub == 1, !g.tiled) or 16x16-cell keys
//                               (g.sub == 16); k_bucket_pols writes every image
//                               pol's records in one value pass (plans with
//                               Plan::pad4)
// Read first: bucket_one (what a record is).  Host side: bucket_part.  The
// fp64 plans' k_bucket_f64 and the work-item kernels are in wstack.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "wstack_fingerprint.h"
#include "wstack_types.h"

namespace sdp {
namespace wstack {

// ------------------------------------------------------------------------
// kernels: geometry and bucketing
// ------------------------------------------------------------------------
// uvw extent: per-block partials (no atomics), reduced by one block after
constexpr int kBoundsBlocks = 1024;

// raw extremes in metres (min/max of su*w, max |u|, max |v|, and min/max of
// the Hermitian-folded su*w: negated on the rows with su*u < 0); the host
// scales them by the frequency range (w*s is monotonic in w for s > 0).
// fpart: the block's two fingerprint words of its rows (wstack_fingerprint.h;
// wrapping sums, so the grid-stride order does not matter)
__global__ __launch_bounds__(256) void k_bounds(const double *__restrict__ uvw, int64_t rs,
                                                int64_t nrow, double su,
                                                double *__restrict__ part,
                                                unsigned long long *__restrict__ fpart) {
    __shared__ double red[6][4];
    __shared__ unsigned long long fred[2][4];
    double wmn = 1e300, wmx = -1e300, umx = 0.0, vmx = 0.0, fmn = 1e300, fmx = -1e300;
    uint64_t fa = 0, fb = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nrow;
         r += (int64_t)gridDim.x * blockDim.x) {
        const double u = uvw[r * rs], v = uvw[r * rs + 1], wr = uvw[r * rs + 2], w = su * wr;
        fp_add_row((uint64_t)r, u, v, wr, fa, fb);
        wmn = fmin(wmn, w);
        wmx = fmax(wmx, w);
        umx = fmax(umx, fabs(u));
        vmx = fmax(vmx, fabs(v));
        const double wf = su * u < 0.0 ? -w : w;
        fmn = fmin(fmn, wf);
        fmx = fmax(fmx, wf);
    }
    for (int o = 32; o > 0; o >>= 1) {
        wmn = fmin(wmn, __shfl_xor(wmn, o));
        wmx = fmax(wmx, __shfl_xor(wmx, o));
        umx = fmax(umx, __shfl_xor(umx, o));
        vmx = fmax(vmx, __shfl_xor(vmx, o));
        fmn = fmin(fmn, __shfl_xor(fmn, o));
        fmx = fmax(fmx, __shfl_xor(fmx, o));
        fa += (uint64_t)__shfl_xor((unsigned long long)fa, o);
        fb += (uint64_t)__shfl_xor((unsigned long long)fb, o);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        fred[0][wv] = fa;
        fred[1][wv] = fb;
        red[0][wv] = wmn;
        red[1][wv] = wmx;
        red[2][wv] = umx;
        red[3][wv] = vmx;
        red[4][wv] = fmn;
        red[5][wv] = fmx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            red[0][0] = fmin(red[0][0], red[0][k]);
            red[1][0] = fmax(red[1][0], red[1][k]);
            red[2][0] = fmax(red[2][0], red[2][k]);
            red[3][0] = fmax(red[3][0], red[3][k]);
            red[4][0] = fmin(red[4][0], red[4][k]);
            red[5][0] = fmax(red[5][0], red[5][k]);
        }
        for (int k = 0; k < 6; ++k) part[k * kBoundsBlocks + blockIdx.x] = red[k][0];
        for (int k = 0; k < 2; ++k)
            fpart[k * kBoundsBlocks + blockIdx.x] = fred[k][0] + fred[k][1] + fred[k][2] + fred[k][3];
    }
}

// out = {min su*w, max su*w, max|u|, max|v|, min freq, max freq, min and max
// of the folded su*w}; fout = the content fingerprint {uvw a, uvw b, freq a,
// freq b} (fingerprint_host computes the same on the host)
__global__ __launch_bounds__(256) void k_bounds_final(int nblocks, const double *__restrict__ part,
                                                      const unsigned long long *__restrict__ fpart,
                                                      const double *__restrict__ freq, int nchan,
                                                      double *__restrict__ out,
                                                      unsigned long long *__restrict__ fout) {
    __shared__ double red[8][256];
    __shared__ unsigned long long fred[4][4];
    double a[8] = {1e300, -1e300, 0.0, 0.0, 1e300, -1e300, 1e300, -1e300};
    uint64_t f[4] = {0, 0, 0, 0};
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        a[0] = fmin(a[0], part[b]);
        a[1] = fmax(a[1], part[kBoundsBlocks + b]);
        a[2] = fmax(a[2], part[2 * kBoundsBlocks + b]);
        a[3] = fmax(a[3], part[3 * kBoundsBlocks + b]);
        a[6] = fmin(a[6], part[4 * kBoundsBlocks + b]);
        a[7] = fmax(a[7], part[5 * kBoundsBlocks + b]);
        f[0] += fpart[b];
        f[1] += fpart[kBoundsBlocks + b];
    }
    for (int c = threadIdx.x; c < nchan; c += 256) {
        a[4] = fmin(a[4], freq[c]);
        a[5] = fmax(a[5], freq[c]);
        fp_add_freq((uint64_t)c, freq[c], f[2], f[3]);
    }
    for (int k = 0; k < 4; ++k) {
        for (int o = 32; o > 0; o >>= 1) f[k] += (uint64_t)__shfl_xor((unsigned long long)f[k], o);
        if ((threadIdx.x & 63) == 0) fred[k][threadIdx.x >> 6] = f[k];
    }
    for (int k = 0; k < 8; ++k) red[k][threadIdx.x] = a[k];
    __syncthreads();
    if (threadIdx.x < 4)
        fout[threadIdx.x] = fred[threadIdx.x][0] + fred[threadIdx.x][1] + fred[threadIdx.x][2] +
                            fred[threadIdx.x][3];
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            const int t = threadIdx.x;
            red[0][t] = fmin(red[0][t], red[0][t + st]);
            red[4][t] = fmin(red[4][t], red[4][t + st]);
            red[6][t] = fmin(red[6][t], red[6][t + st]);
            for (int k : {1, 2, 3, 5, 7}) red[k][t] = fmax(red[k][t], red[k][t + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 8) out[threadIdx.x] = red[threadIdx.x][0];
}

// per-part plan metadata (one buffer, one D2H copy when the host needs it):
// {nbad lo, nbad hi, nrec, nitems, first item of each first-plane value
// [nps + 1]}; meta[3] is also the item count persistent launches read
__global__ void k_part_meta(const unsigned long long *__restrict__ nbad,
                            const unsigned *__restrict__ nrec, const unsigned *__restrict__ npad,
                            const unsigned *__restrict__ ioffs, int groups_per_plane, int nps,
                            unsigned *__restrict__ meta) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) {
        meta[0] = (unsigned)(*nbad & 0xffffffffull);
        meta[1] = (unsigned)(*nbad >> 32);
        meta[2] = *nrec - (npad ? *npad : 0u);  // gridded visibilities (pads excluded)
        meta[3] = ioffs[(size_t)nps * groups_per_plane];
    }
    if (k <= nps) meta[4 + k] = ioffs[(size_t)k * groups_per_plane];
}

// Wave-level run-length aggregation: consecutive lanes with equal keys share
// one atomic on counter[key]; with kScatter each lane gets its slot.
template <bool kScatter>
__device__ __forceinline__ unsigned run_reserve(unsigned key, bool valid, unsigned *counter) {
    const int lane = threadIdx.x & 63;
    const unsigned prev = __shfl_up(key, 1);
    const bool start = (lane == 0) || (prev != key);
    const unsigned long long B = __ballot(start);
    const unsigned long long above = (lane == 63) ? 0ull : (B & ~((2ull << lane) - 1ull));
    const int end = above ? (__ffsll((long long)above) - 1) : 64;
    unsigned base = 0;
    if (valid && start) base = atomicAdd(&counter[key], (unsigned)(end - lane));
    if (!kScatter) return 0;
    const unsigned long long upto = (lane == 63) ? B : (B & ((2ull << lane) - 1ull));
    const int head = 63 - __clzll((long long)upto);
    const unsigned hb = __shfl(base, head);
    return hb + (unsigned)(lane - head);
}

// Visibility-side prologue fused into the bucketing pass (sdp_hip_ms2dirty_vis,
// SURVEY.md §8(f) rank 2): flag masking of the visibilities and weights,
// fp64 weights, the polarisation-frame conversion of the reference's
// convert_pol_frame (imaging/ng.py:193-198) as one row of its matrix, and
// the weight sum the reference takes with numpy.sum (ng.py:258, :289).
struct VisExtra {
    int64_t vps = 0;           // vis pol stride (elements); vis points at pol 0 when conv
    int npv = 1;               // vis pols combined
    bool conv = false;         // vis_eff = sum_k coef_k * vis_k * (1 - flag_k)
    double cre[4] = {1.0, 0.0, 0.0, 0.0}, cim[4] = {0.0, 0.0, 0.0, 0.0};
    int wgt_f64 = 0;           // weights are f64 (else f32)
    const void *flags = nullptr;
    int fbytes = 0;            // 1 / 4 / 8 byte integer flags at pol 0
    int64_t frs = 0, fcs = 0, fps = 0;
    int fpol = 0;              // pol whose flag masks the weight (and the vis when !conv)
    double *sumwt = nullptr;   // += sum of the effective weights (device, may be null)
    // shift_vis_to_image with tangent=True (reference imaging/base.py:48-92,
    // visibility/base.py:27-45, :60-90): phase d = uvw_lambda . (l, m, n-1)
    // in turns, folded into the record factor as exp(+2 pi i d) for invert
    // (vis * conj(phasor)) and exp(-2 pi i d) for predict (vis * phasor)
    bool shift = false;
    double sl = 0.0, sm = 0.0, sn = 0.0;
    // SDP_HIP_KEEP_BUCKETS: every in-grid visibility is bucketed (zero
    // weights add exact zeros), so the bucketing holds for any weights
    bool all = false;
};

constexpr int kSumSlots = 1024;

__device__ __forceinline__ double flag_mask(const VisExtra &x, int64_t row, int chan, int pol) {
    const int64_t i = row * x.frs + chan * x.fcs + pol * x.fps;
    double f;
    if (x.fbytes == 8) f = (double)static_cast<const int64_t *>(x.flags)[i];
    else if (x.fbytes == 4) f = (double)static_cast<const int32_t *>(x.flags)[i];
    else f = (double)static_cast<const int8_t *>(x.flags)[i];
    return 1.0 - f;
}

__device__ __forceinline__ double eff_weight(const void *wgt, int64_t wrs, int64_t wcs,
                                             const VisExtra &x, int64_t row, int chan) {
    double w = 1.0;
    if (wgt) {
        const int64_t i = row * wrs + chan * wcs;
        w = x.wgt_f64 ? static_cast<const double *>(wgt)[i]
                      : (double)static_cast<const float *>(wgt)[i];
    }
    // select, not multiply: a flagged sample's weight is an exact zero even
    // when the stored weight is NaN or Inf (ducc0 skips zero-weight samples)
    if (x.fbytes) {
        const double m = flag_mask(x, row, chan, x.fpol);
        w = m == 0.0 ? 0.0 : w * m;
    }
    return w;
}

__device__ __forceinline__ double2 load_vis_d(const float2 *p) {
    const float2 v = *p;
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ double2 load_vis_d(const double2 *p) { return *p; }

__device__ __forceinline__ float2 load_vis(const float2 *p) { return *p; }
__device__ __forceinline__ float2 load_vis(const double2 *p) {
    const double2 v = *p;
    return make_float2((float)v.x, (float)v.y);
}

// Two passes over the visibilities.  Rank pass (kScatter = false): fp64
// coordinates -> bucket key, and the visibility's rank inside its bucket
// from a run-aggregated atomicAdd on the histogram; the rank is stored.
// Scatter pass: position = offs[key] + rank -- no atomics -- and the 32-byte
// record is written there.  Invalid visibilities carry key 0xffffffff.
template <class VT>
__device__ __forceinline__ float2 eff_vis(const VT *vis, int64_t vrs, int64_t vcs,
                                          const VisExtra &x, int64_t row, int chan) {
    const VT *p = vis + row * vrs + chan * vcs;
    // flagged pols contribute exact zeros (select, not multiply: a NaN in a
    // flagged visibility must not reach the image)
    if (!x.conv) {
        if (!x.fbytes) return load_vis(p);
        const double m = flag_mask(x, row, chan, x.fpol);
        if (m == 0.0) return make_float2(0.0f, 0.0f);
        const double2 v = load_vis_d(p);
        return make_float2((float)(v.x * m), (float)(v.y * m));
    }
    double re = 0.0, im = 0.0;
    for (int k = 0; k < x.npv; ++k) {
        if (x.cre[k] == 0.0 && x.cim[k] == 0.0) continue;
        double m = 1.0;
        if (x.fbytes) {
            m = flag_mask(x, row, chan, k);
            if (m == 0.0) continue;
        }
        double2 v = load_vis_d(p + k * x.vps);
        v.x *= m;
        v.y *= m;
        re += x.cre[k] * v.x - x.cim[k] * v.y;
        im += x.cre[k] * v.y + x.cim[k] * v.x;
    }
    return make_float2((float)re, (float)im);
}

template <class T>
struct TypeTag {
    using type = T;
};

// Runtime value -> template argument: calls f(std::integral_constant<int, k>{})
// with k = v for v in [Lo, Hi) and k = Hi for every other v, so f's body is
// instantiated for exactly Lo .. Hi.
template <int Lo, int Hi, class F>
inline void dispatch_int(int v, F &&f) {
    if constexpr (Lo < Hi) {
        if (v != Lo) return dispatch_int<Lo + 1, Hi>(v, f);
    }
    f(std::integral_constant<int, Lo>{});
}

template <class VT>
__device__ __forceinline__ double2 eff_vis_d(const VT *vis, int64_t vrs, int64_t vcs,
                                             const VisExtra &x, int64_t row, int chan) {
    const VT *p = vis + row * vrs + chan * vcs;
    if (!x.conv) {
        if (!x.fbytes) return load_vis_d(p);
        const double m = flag_mask(x, row, chan, x.fpol);
        if (m == 0.0) return make_double2(0.0, 0.0);
        const double2 v = load_vis_d(p);
        return make_double2(v.x * m, v.y * m);
    }
    double re = 0.0, im = 0.0;
    for (int k = 0; k < x.npv; ++k) {
        if (x.cre[k] == 0.0 && x.cim[k] == 0.0) continue;
        double m = 1.0;
        if (x.fbytes) {
            m = flag_mask(x, row, chan, k);
            if (m == 0.0) continue;
        }
        double2 v = load_vis_d(p + k * x.vps);
        v.x *= m;
        v.y *= m;
        re += x.cre[k] * v.x - x.cim[k] * v.y;
        im += x.cre[k] * v.y + x.cim[k] * v.x;
    }
    return make_double2(re, im);
}

struct TLoad {
    uint32_t row, chan;
    double um, vm, wm, s, wd;  // s = frequency / c (fsc[chan]: the same division as vis_coord)
    double keep;               // 1 - flag of the weight's pol (1 without flags)
    bool live;
};

// The weight and flag element types are compile-time in the bucketing
// passes -- WT: 4 = f32, 8 = f64 (no weights: a device 1.0f with zero
// strides); FB: 0 = no flags, 1 = int8, 8 = int64 flags (int32 flags are
// widened to int64 first, k_widen_flags) -- and a lane's visibilities load
// from clamped, in-bounds indices with no branch before their first use:
// all of a lane's visibilities' loads (uvw, frequency scale, weight, flag,
// and in the value pass the visibility) are in flight together.  A runtime switch on the
// types, with each load behind its own branch and a `live` test, had put a
// wait for every load before the next one issued (C2 count pass: ~200
// instructions and four serialised memory round trips per visibility).
template <int WT, int FB>
__device__ __forceinline__ TLoad t_load(const Geo &g, int64_t v, int64_t vend,
                                        const double *__restrict__ uvw, int64_t rs,
                                        const double *__restrict__ fsc,
                                        const void *__restrict__ wgt, int64_t wrs, int64_t wcs,
                                        const VisExtra &x) {
    TLoad L;
    L.live = v < vend;
    const uint32_t v32 = (uint32_t)(L.live ? v : vend - 1), nc = (uint32_t)g.nchan;
    // row = v / nchan through the fp64 reciprocal (exact to one step, then
    // corrected), not an integer division
    uint32_t r32 = (uint32_t)((double)v32 * g.inv_nchan);
    if ((uint64_t)r32 * nc > v32) --r32;
    else if ((uint64_t)(r32 + 1u) * nc <= v32) ++r32;
    L.row = r32;
    L.chan = v32 - r32 * nc;
    const double *p = uvw + (int64_t)L.row * rs;
    L.um = p[0];
    L.vm = p[1];
    L.wm = p[2];
    L.s = fsc[L.chan];
    double w;
    const int64_t wi = (int64_t)L.row * wrs + (int64_t)L.chan * wcs;
    if constexpr (WT == 8) w = static_cast<const double *>(wgt)[wi];
    else w = (double)static_cast<const float *>(wgt)[wi];
    L.keep = 1.0;
    if constexpr (FB != 0) {
        using FT = typename std::conditional<FB == 8, int64_t, int8_t>::type;
        L.keep = 1.0 - (double)static_cast<const FT *>(
                           x.flags)[(int64_t)L.row * x.frs + (int64_t)L.chan * x.fcs + x.fpol * x.fps];
        // select, not multiply: a flagged sample's weight is an exact zero
        // even when the stored weight is NaN or Inf
        w = L.keep == 0.0 ? 0.0 : w * L.keep;
    }
    L.wd = L.live ? w : 0.0;
    return L;
}

// int32 flags of a two-level pass as int64 (FB = 8): a contiguous
// [nrow, nchan, npol] copy (one element for a zero-stride broadcast)
__device__ float g_unit_weight = 1.0f;  // the weights of a call without weights
template <class FT>
__global__ void k_widen_flags(const FT *__restrict__ src, int64_t frs, int64_t fcs, int64_t fps,
                              int64_t nrow, int nchan, int npol, int64_t *__restrict__ dst) {
    const int64_t n = nrow * nchan * (int64_t)npol;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rc = i / npol, row = rc / nchan;
        const int pol = (int)(i - rc * npol), chan = (int)(rc - row * nchan);
        dst[i] = (int64_t)src[row * frs + chan * fcs + pol * fps];
    }
}

// A pol conversion's visibility (x.conv) for the typed passes: every used
// pol's value and flag are loaded before any is combined.  The generic
// eff_vis / eff_vis_d load a pol's flag, branch on it and only then load its
// value, pol after pol -- serialised memory round trips (the 4-pol MFS value
// pass ran at 1.5 TB/s).  Coefficients are uniform, flags selected, not
// multiplied: a NaN in a flagged pol must not reach the image.
template <class VT, int FB>
__device__ __forceinline__ double2 conv_vis(const VT *vis, int64_t vrs, int64_t vcs,
                                            const VisExtra &x, uint32_t row, uint32_t chan) {
    using FT = typename std::conditional<FB == 8, int64_t, int8_t>::type;
    const VT *p = vis + (int64_t)row * vrs + (int64_t)chan * vcs;
    VT v[4];
    FT f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = VT{};
        f[k] = 0;
        if (k < x.npv && (x.cre[k] != 0.0 || x.cim[k] != 0.0)) {
            v[k] = p[k * x.vps];
            if constexpr (FB != 0)
                f[k] = static_cast<const FT *>(
                    x.flags)[(int64_t)row * x.frs + (int64_t)chan * x.fcs + k * x.fps];
        }
    }
    double re = 0.0, im = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < x.npv && (x.cre[k] != 0.0 || x.cim[k] != 0.0)) {
            const double m = 1.0 - (double)f[k];
            const double vx = m == 0.0 ? 0.0 : (double)v[k].x * m;
            const double vy = m == 0.0 ? 0.0 : (double)v[k].y * m;
            re += x.cre[k] * vx - x.cim[k] * vy;
            im += x.cre[k] * vy + x.cim[k] * vx;
        }
    }
    return make_double2(re, im);
}

// the visibility's value in two phases: `load` issues the loads (the
// visibility from clamped indices, beside the lane's other loads), `value`
// combines them after every load is in flight.  Without a pol conversion the
// weight pol's flag (TLoad::keep) masks it; a pol conversion (x.conv, the
// 4-pol frames) reads its pols and flags in `value`.
template <class VT, int KIND, bool kGrid, int FB>
struct TVal {
    using type = typename std::conditional<KIND >= 2, double2, float2>::type;
    __device__ static __forceinline__ VT load(const VT *vis, int64_t vrs, int64_t vcs,
                                              const VisExtra &x, const TLoad &L) {
        VT raw{};
        if constexpr (kGrid)
            if (vis && !x.conv) raw = vis[(int64_t)L.row * vrs + (int64_t)L.chan * vcs];
        return raw;
    }
    __device__ static __forceinline__ type value(const VT *vis, int64_t vrs, int64_t vcs,
                                                 const VisExtra &x, const TLoad &L, VT raw) {
        type xv;
        xv.x = 1;
        xv.y = 0;
        if constexpr (kGrid) {
            if (!vis) return xv;  // (unit visibilities: the PSF)
            if (x.conv) {
                const double2 d = conv_vis<VT, FB>(vis, vrs, vcs, x, L.row, L.chan);
                xv.x = d.x;
                xv.y = d.y;
                return xv;
            }
            const double2 v = make_double2((double)raw.x, (double)raw.y);
            if constexpr (FB == 0) {
                xv.x = v.x;
                xv.y = v.y;
            } else {
                // select, not multiply: a NaN in a flagged visibility must not
                // reach the image
                const double m = L.keep;
                xv.x = m == 0.0 ? 0.0 : v.x * m;
                xv.y = m == 0.0 ? 0.0 : v.y * m;
            }
        }
        return xv;
    }
};

// One visibility of k_bucket (single-level bucketing: the fp32 predict, kept
// buckets, large grids).  Its loads -- uvw, frequency scale, weight, flag,
// and in the value pass its rank and visibility -- are issued together from
// clamped indices (t_load<WT, FB>, TVal), before any of them is used.
template <class VT, bool kScatter, bool kGrid, bool kCompact, int WT, int FB>
__device__ __forceinline__ void bucket_one(const Geo &g, int64_t v, int64_t nvis,
                                           const double *__restrict__ uvw, int64_t uvw_rs,
                                           const double *__restrict__ fsc,
                                           const VT *__restrict__ vis, int64_t vrs, int64_t vcs,
                                           const void *__restrict__ wgt, int64_t wrs,
                                           int64_t wcs, const VisExtra &x, double *sw_slots,
                                           unsigned *counter, unsigned *__restrict__ rk,
                                           VisRec *__restrict__ recs, unsigned long long *nbad,
                                           uint8_t *__restrict__ cls, float2 *__restrict__ zout) {
    using V = TVal<VT, kCompact ? 0 : 1, kGrid, FB>;
    const TLoad L = t_load<WT, FB>(g, v, nvis, uvw, uvw_rs, fsc, wgt, wrs, wcs, x);
    const int64_t vg = (int64_t)L.row * g.nchan + L.chan;  // row * nchan + chan
    // (a w-slab call's outsiders: no rank stored, no weight summed)
    const bool outside = L.live && g.slab && slab_out_v(g, L.wm, L.s);
    const double wd = outside ? 0.0 : L.wd;
    const float wt = (float)wd;
    if (kScatter) {
        const unsigned mine = rk[vg];
        const VT raw = V::load(vis, vrs, vcs, x, L);
        if (sw_slots) {
            // weight sum of a reused bucketing (SDP_HIP_REUSE_BUCKETS): the
            // count pass did not run, so the value pass sums the weights
            double ws = wd;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o, 64);
            if ((threadIdx.x & 63) == 0 && ws != 0.0)
                atomicAdd(&sw_slots[(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) &
                                    (kSumSlots - 1)],
                          ws);
        }
        if (!L.live || outside || mine == 0xffffffffu) return;
        const Coord c = vis_coord_v(g, L.um, L.vm, L.wm, L.s);
        const unsigned pos = counter[coord_key(g, c, L.row)] + mine;
        float cr = wt, ci = 0.0f;
        if (kGrid) {
            // a zero-weight sample (bucketed only by a SDP_HIP_KEEP_BUCKETS
            // plan, for the other pols) is an exact zero whatever its
            // visibility holds
            const float2 xv = V::value(vis, vrs, vcs, x, L, raw);
            cr = wt != 0.0f ? xv.x * wt : 0.0f;
            ci = wt != 0.0f ? xv.y * wt : 0.0f;
        }
        if (g.do_w || x.shift) {
            double ph = g.do_w ? c.w * g.s0 : 0.0;
            if (x.shift) ph += (L.um * x.sl + L.vm * x.sm + L.wm * x.sn) * L.s;
            ph -= rint(ph);
            float sn, cs;
            sincospif((float)(2.0 * ph), &sn, &cs);
            if (!kGrid) sn = -sn;
            const float r_ = cr * cs - ci * sn, i_ = cr * sn + ci * cs;
            cr = r_;
            ci = i_;
        }
        if (kGrid && c.conj) ci = -ci;  // (folded: after the rotation)
        if (kCompact) {
            // RecC: offsets as fractions of (1 - W/2) - offset (do_w off: w = 0)
            const double base = 1.0 - 0.5 * g.W;
            const uint32_t qu = fix_frac(base - c.du, 21), qv = fix_frac(base - c.dv, 21);
            const uint32_t qw = g.do_w ? fix_frac(base - c.dw, 22) : 0u;
            RecC rc;
            rc.cre = cr;
            rc.cim = ci;
            rc.lo = qu | (qv << 21);
            rc.hi = (qv >> 11) | (qw << 10);
            reinterpret_cast<RecC *>(recs)[pos] = rc;
            // large grids (16x16-cell buckets): the record's cell in its
            // bucket, for the padded sub-sort (k_subsort_pad)
            if (cls) cls[pos] = (uint8_t)(((c.ic0 & 15) >> 1) * 32 + (c.jc0 & 15) * 2 + (c.ic0 & 1));
            return;
        }
        VisRec rec;
        rec.cre = cr;
        rec.cim = ci;
        rec.fu = c.fu;
        rec.fv = c.fv;
        rec.fw = c.fw;
        rec.ij = (uint32_t)c.ic0 | ((uint32_t)c.jc0 << 16);
        rec.p0 = (uint32_t)c.p0;
        rec.idx = (uint32_t)vg;
        recs[pos] = rec;
        return;
    }
    // rank pass
    bool valid = L.live && !outside && (x.all || wt != 0.0f);
    Coord c;
    c.ok = false;
    if (valid) {
        c = vis_coord_v(g, L.um, L.vm, L.wm, L.s);
        if (!c.ok) {
            valid = false;
            if (!c.skip) atomicAdd(nbad, 1ull);
        }
    }
    const unsigned key = valid ? coord_key(g, c, L.row) : 0xffffffffu;
    const unsigned rank = run_reserve<true>(key, valid, counter);
    // only the rank is kept: the scatter pass recomputes the key
    if (L.live && !outside) rk[vg] = valid ? rank : 0xffffffffu;
    // a predict writing its visibilities in place zeroes the ones no record
    // reaches here (the degridder writes every other one)
    if (zout && L.live && !valid) zout[vg] = make_float2(0.0f, 0.0f);
    if (sw_slots) {
        // weight sum: wave reduction, one atomic per wave into a slot
        double ws = wd;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o, 64);
        if ((threadIdx.x & 63) == 0 && ws != 0.0)
            atomicAdd(&sw_slots[(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) &
                                (kSumSlots - 1)],
                      ws);
    }
}

template <class VT, bool kScatter, bool kGrid, bool kCompact, int WT, int FB>
__global__ void k_bucket(Geo g, int64_t nvis, const double *__restrict__ uvw, int64_t uvw_rs,
                         const double *__restrict__ fsc, const VT *__restrict__ vis, int64_t vrs,
                         int64_t vcs, const void *__restrict__ wgt, int64_t wrs, int64_t wcs,
                         VisExtra x, double *sw_slots, unsigned *counter, unsigned *__restrict__ rk,
                         VisRec *__restrict__ recs, unsigned long long *nbad,
                         uint8_t *__restrict__ cls, float2 *__restrict__ zout) {
    bucket_one<VT, kScatter, kGrid, kCompact, WT, FB>(
        g, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nvis, uvw, uvw_rs, fsc, vis, vrs, vcs,
        wgt, wrs, wcs, x, sw_slots, counter, rk, recs, nbad, cls, zout);
}

// The image pols of one invert_ng call sharing one bucketing
// (sdp_hip_ms2dirty_vis_pols): image pol q takes row q of the conversion
// matrix over the visibility pols, the weights of pol q masked by the flags
// of pol q, and its own record array.
struct PolsSpec {
    int npo = 0;                              // image pols (<= 4)
    double cre[4][4] = {}, cim[4][4] = {};    // [image pol][vis pol]
    const void *wgt = nullptr;                // weights [row, chan, pol]
    int64_t wrs = 0, wcs = 0, wps = 0;
    RecC *recs[4] = {};
    double *slots[4] = {};                    // weight-sum slots per image pol, or null
};

// The value pass of all image pols at once (one-cell 4-padded plans): each
// visibility's pols, flags and weights are read once and the npo records
// written at the one position the shared bucketing gives it.  One pass per
// image pol read the pol-interleaved visibilities, flags and weights whole
// every time (their cache lines) -- the 4-pol MFS value passes ran 5.7 ms
// each on C2.  The values are those of the per-pol pass bit for bit: the
// conversion sum in fp64 rounded to fp32, times the fp32 masked weight, then
// the record factor.
template <class VT, int WT, int FB, int NPO>
__global__ __launch_bounds__(256) void k_bucket_pols(Geo g, int64_t nvis,
                                                     const double *__restrict__ uvw,
                                                     int64_t uvw_rs,
                                                     const double *__restrict__ fsc,
                                                     const VT *__restrict__ vis, int64_t vrs,
                                                     int64_t vcs, VisExtra x, PolsSpec ps,
                                                     const unsigned *__restrict__ counter,
                                                     const unsigned *__restrict__ rk) {
    using FT = typename std::conditional<FB == 8, int64_t, int8_t>::type;
    using WTT = typename std::conditional<WT == 8, double, float>::type;
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    // (t_load's weight and flag are pol 0's; the loop below reads every pol's)
    const TLoad L = t_load<WT, FB>(g, v, nvis, uvw, uvw_rs, fsc, ps.wgt, ps.wrs, ps.wcs, x);
    const int64_t vg = (int64_t)L.row * g.nchan + L.chan;
    const bool outside = L.live && g.slab && slab_out_v(g, L.wm, L.s);
    // every load of the visibility before any use
    const unsigned mine = rk[vg];
    const VT *pv = vis + (int64_t)L.row * vrs + (int64_t)L.chan * vcs;
    VT vv[4];
    FT ff[4];
    WTT ww[NPO];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        vv[k] = VT{};
        ff[k] = 0;
        if (k < x.npv) {
            vv[k] = pv[k * x.vps];
            if constexpr (FB != 0)
                ff[k] = static_cast<const FT *>(
                    x.flags)[(int64_t)L.row * x.frs + (int64_t)L.chan * x.fcs + k * x.fps];
        }
    }
#pragma unroll
    for (int q = 0; q < NPO; ++q)
        ww[q] = static_cast<const WTT *>(
            ps.wgt)[(int64_t)L.row * ps.wrs + (int64_t)L.chan * ps.wcs + q * ps.wps];
    // the masked weights (select: a flagged sample's weight is an exact zero
    // even when the stored weight is NaN or Inf) and their sums
    double wd[NPO];
#pragma unroll
    for (int q = 0; q < NPO; ++q) {
        double w = (double)ww[q];
        if constexpr (FB != 0) {
            const double keep = 1.0 - (double)ff[q];
            w = keep == 0.0 ? 0.0 : w * keep;
        }
        wd[q] = (L.live && !outside) ? w : 0.0;
        if (ps.slots[q]) {
            double ws = wd[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o, 64);
            if ((threadIdx.x & 63) == 0 && ws != 0.0)
                atomicAdd(&ps.slots[q][(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) &
                                       (kSumSlots - 1)],
                          ws);
        }
    }
    if (!L.live || outside || mine == 0xffffffffu) return;
    const Coord c = vis_coord_v(g, L.um, L.vm, L.wm, L.s);
    const unsigned pos = counter[coord_key(g, c, L.row)] + mine;
    float sn = 0.0f, cs = 1.0f;
    const bool rot = g.do_w || x.shift;
    if (rot) {
        double ph = g.do_w ? c.w * g.s0 : 0.0;
        if (x.shift) ph += (L.um * x.sl + L.vm * x.sm + L.wm * x.sn) * L.s;
        ph -= rint(ph);
        sincospif((float)(2.0 * ph), &sn, &cs);
    }
    const double base = 1.0 - 0.5 * g.W;
    const uint32_t qu = fix_frac(base - c.du, 21), qv = fix_frac(base - c.dv, 21);
    const uint32_t qw = g.do_w ? fix_frac(base - c.dw, 22) : 0u;
#pragma unroll
    for (int q = 0; q < NPO; ++q) {
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < x.npv && (ps.cre[q][k] != 0.0 || ps.cim[q][k] != 0.0)) {
                double m = 1.0;
                if constexpr (FB != 0) m = 1.0 - (double)ff[k];
                const double vx = m == 0.0 ? 0.0 : (double)vv[k].x * m;
                const double vy = m == 0.0 ? 0.0 : (double)vv[k].y * m;
                re += ps.cre[q][k] * vx - ps.cim[q][k] * vy;
                im += ps.cre[q][k] * vy + ps.cim[q][k] * vx;
            }
        }
        const float wt = (float)wd[q];
        const float xr = (float)re, xi = (float)im;
        const float cr = wt != 0.0f ? xr * wt : 0.0f, ci = wt != 0.0f ? xi * wt : 0.0f;
        RecC rc;
        rc.cre = rot ? cr * cs - ci * sn : cr;
        rc.cim = rot ? cr * sn + ci * cs : ci;
        if (c.conj) rc.cim = -rc.cim;  // (folded: after the rotation)
        rc.lo = qu | (qv << 21);
        rc.hi = (qv >> 11) | (qw << 10);
        ps.recs[q][pos] = rc;
    }
}

}  // namespace wstack
}  // namespace sdp
