// Multi-scale multi-frequency CLEAN minor cycles for gfx950 (Rau & Cornwell
// 2011, Algorithm 1): sdp_hip_mfsclean_plane runs up to niter cycles on one
// polarisation without leaving the device, restating the loops of the
// reference's
//   msmfsclean                                 image/cleaners.py:831-876
//   find_global_optimum                        cleaners.py:901-974
//   update_scale_moment_residual               cleaners.py:977-1001
//   update_moment_model                        cleaners.py:1004-1031
//   calculate_scale_moment_principal_solution  cleaners.py:1107-1121
//   find_optimum_scale_zero_moment             cleaners.py:1124-1157
// (the set-up -- scale stacks, FFT convolutions, Hessians, window stack -- is
// the Python layer's).
//
// The structure is clean.hip's.  A cycle is two plain stream-ordered kernels:
//   k_select  one workgroup reduces the cached per-(scale, tile) maxima to the
//             next (scale, pixel), forms mval = the principal solution there,
//             counts the cycle and applies the stop test, which comes before
//             the update;
//   k_update  a grid sized by the PSF box.  Slice z < S updates scale z: it
//             reads the T residual moments of its tile's pixels and the
//             2T - 1 PSF planes of (mscale, z), writes the T new residuals,
//             forms the search value from them in registers and refreshes the
//             tile's cached maxima.  Slices S .. S + T - 1 add the scale
//             kernel to the T model planes over the kernel's extent.
// Tiles the patch does not touch keep their cached maxima.  The host enqueues
// cycles in batches and reads the stop flag once per batch; kernels launched
// after the stop return at once.  No grid-wide barrier, no spinning.
//
// The scale-scale-moment-moment PSF is stored as its 2T - 1 distinct planes:
// plane k of [S, S, 2T - 1, pny, pnx] is the reference's ssmmpsf[s, p, t, q]
// for every t + q = k (it keeps T^2 copies).
//
// Arithmetic is fp64 with contraction off, in the order numpy's einsum takes
// (plain left-to-right accumulation):
//   sol[s, n] = ((ihs[s, 0, n] * r[s, 0]) + ihs[s, 1, n] * r[s, 1]) + ...
//   r[s, t]  -= gain * (((P[t + 0] * mval[0]) + P[t + 1] * mval[1]) + ...)
//   m[t]     += (kernel * gain) * mval[t]
//   CASA: for m1: d += (2 * sol[m1]) * r[m1]; for m2: d -= (hs[m1, m2] * sol[m1]) * sol[m2]
//
// The search keeps find_optimum_scale_zero_moment's quirk: per scale the
// pixel is numpy.argmax |field[s]| WITHOUT window or sensitivity (first
// maximum in row-major order; every reduction level breaks ties on the lower
// flat index), while the scales are compared on max |field[s] * window[s] *
// sensitivity| with a strict '>' from 0.0 at (0, 0, scale 0).  So the tile
// cache holds two entries: the unweighted (value, index) and the weighted
// value.  NaN search values are never selected.
#include "sdp_common.h"

#include <climits>
#include <cmath>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace sdp {
namespace mfsclean {

constexpr int kThreads = 256;
constexpr int kTileX = 64;  // one wave reads one 512-byte row segment
constexpr int kTileY = 16;
constexpr int kSelThreads = 1024;
constexpr int kMaxScales = 16;
constexpr int kMaxMoments = 4;
constexpr int kHess = 2 * kMaxMoments * kMaxMoments;  // doubles per scale: hs then ihs, [4][4] each
constexpr int kBatch = 32;  // cycles enqueued between two reads of the stop flag

struct State {
    int done;    // stop decided by k_select
    int active;  // the next k_update has work
    int iter;    // cycles counted as the reference counts them
    int reason;  // SDP_HIP_CLEAN_STOP_*
    int peak_y, peak_x, peak_s, pad;
    double mval[kMaxMoments];
    int counts[kMaxScales];
};

struct Params {
    int ns, nt, ny, nx, pny, pnx;
    int ntx, nty;  // tiles per image plane
    int kext;      // scale kernels vanish beyond this many pixels from the PSF origin (0: unknown)
    int casa;      // the search field is dchisq instead of sol[., 0]
    double gain, absthresh;
};

struct Best {
    double key;
    int idx;
};

__device__ __forceinline__ bool better(double k1, int i1, double k2, int i2) {
    return k1 > k2 || (k1 == k2 && i1 < i2);
}

__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k = __shfl_xor(b.key, o, 64);
        const int i = __shfl_xor(b.idx, o, 64);
        if (better(k, i, b.key, b.idx)) b = {k, i};
    }
    return b;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k = __shfl_xor(v, o, 64);
        if (k > v) v = k;
    }
    return v;
}

// The principal solution sol[n] of one pixel of one scale (cleaners.py:1119)
// and the search field made from it: sol[0], or CASA's dchisq (:943-956).
// h: the scale's hs [4][4] then ihs [4][4].
template <int T>
__device__ __forceinline__ double search_field(const double (&r)[T], const double *__restrict__ h,
                                               int casa, double (&sol)[T]) {
    const double *hs = h, *ihs = h + kMaxMoments * kMaxMoments;
#pragma unroll
    for (int n = 0; n < T; ++n) {
        double acc = ihs[n] * r[0];
#pragma unroll
        for (int m = 1; m < T; ++m) acc = acc + ihs[m * kMaxMoments + n] * r[m];
        sol[n] = acc;
    }
    if (!casa) return sol[0];
    double d = 0.0;
#pragma unroll
    for (int m1 = 0; m1 < T; ++m1) {
        d = d + (2.0 * sol[m1]) * r[m1];
#pragma unroll
        for (int m2 = 0; m2 < T; ++m2) d = d - (hs[m1 * kMaxMoments + m2] * sol[m1]) * sol[m2];
    }
    return d;
}

struct Box {
    int y0, y1, x0, x1;
};

// overlapIndices: [peak - n//2, peak + n//2) clipped to the image; PSF pixel
// n//2 sits on the peak.
__device__ __forceinline__ Box patch_box(const Params &p, int py, int px) {
    const int hy = p.pny / 2, hx = p.pnx / 2;
    return {max(0, py - hy), min(p.ny, py + hy), max(0, px - hx), min(p.nx, px + hx)};
}

// blockIdx.z < ns: residual scale z.  blockIdx.z >= ns: model moment z - ns.
// init: every tile of the image, no subtraction (launched with ns slices).
template <int T>
__global__ __launch_bounds__(kThreads) void k_update(Params p, int init, const State *st,
                                                     double *res, const double *__restrict__ psf,
                                                     const double *__restrict__ win,
                                                     const double *__restrict__ sens,
                                                     const double *__restrict__ skern,
                                                     const double *__restrict__ hess, double *model,
                                                     double *tkey, int *tidx, double *twkey) {
    int ty = blockIdx.y, tx = blockIdx.x;
    int py = 0, px = 0, ms = 0;
    double mval[T];
#pragma unroll
    for (int t = 0; t < T; ++t) mval[t] = 0.0;
    Box b{0, 0, 0, 0};
    const int s = blockIdx.z;
    if (!init) {
        if (!st->active) return;
        py = st->peak_y;
        px = st->peak_x;
        ms = st->peak_s;
#pragma unroll
        for (int t = 0; t < T; ++t) mval[t] = st->mval[t];
        b = patch_box(p, py, px);
        if (s >= p.ns && p.kext > 0)  // the model slices visit the kernel's support only
            b = {max(b.y0, py - p.kext), min(b.y1, py + p.kext + 1), max(b.x0, px - p.kext),
                 min(b.x1, px + p.kext + 1)};
        ty += b.y0 / kTileY;
        tx += b.x0 / kTileX;
        if (ty > (b.y1 - 1) / kTileY || tx > (b.x1 - 1) / kTileX) return;
    }
    const int hy = p.pny / 2, hx = p.pnx / 2;
    const size_t plane = (size_t)p.ny * p.nx, pplane = (size_t)p.pny * p.pnx;
    const int x = tx * kTileX + (threadIdx.x & 63);

    if (s >= p.ns) {
        // m_model[t, patch] += scale kernel * gain * mval[t] (cleaners.py:1025-1029)
        const int t = s - p.ns;
        const double mv = st->mval[t];
        double *m = model + (size_t)t * plane;
#pragma unroll
        for (int k = 0; k < kTileY / 4; ++k) {
            const int y = ty * kTileY + (threadIdx.x >> 6) + 4 * k;
            if (y < b.y0 || y >= b.y1 || x < b.x0 || x >= b.x1) continue;
            const size_t pix = (size_t)y * p.nx + x;
            const size_t ppix = (size_t)(hy + y - py) * p.pnx + (hx + x - px);
            m[pix] = m[pix] + (skern[(size_t)ms * pplane + ppix] * p.gain) * mv;
        }
        return;
    }

    const double *h = hess + (size_t)s * kHess;
    const bool weighted = win || sens;
    double *rs = res + (size_t)s * T * plane;
    const double *ps = psf + ((size_t)ms * p.ns + s) * (2 * T - 1) * pplane;
    Best best{-1.0, INT_MAX};
    double wbest = -1.0;
#pragma unroll
    for (int k = 0; k < kTileY / 4; ++k) {
        const int y = ty * kTileY + (threadIdx.x >> 6) + 4 * k;
        if (y >= p.ny || x >= p.nx) continue;
        const size_t pix = (size_t)y * p.nx + x;
        double r[T];
#pragma unroll
        for (int t = 0; t < T; ++t) r[t] = rs[t * plane + pix];
        if (y >= b.y0 && y < b.y1 && x >= b.x0 && x < b.x1) {
            const size_t ppix = (size_t)(hy + y - py) * p.pnx + (hx + x - px);
            double pk[2 * T - 1];
#pragma unroll
            for (int j = 0; j < 2 * T - 1; ++j) pk[j] = ps[j * pplane + ppix];
            // smresidual[s, t, patch] -= gain * sum_q ssmmpsf[mscale, s, t, q] * mval[q]
            // (cleaners.py:995-999)
#pragma unroll
            for (int t = 0; t < T; ++t) {
                double acc = pk[t] * mval[0];
#pragma unroll
                for (int q = 1; q < T; ++q) acc = acc + pk[t + q] * mval[q];
                r[t] = r[t] - p.gain * acc;
                rs[t * plane + pix] = r[t];
            }
        }
        double sol[T];
        const double field = search_field<T>(r, h, p.casa, sol);
        const double key = fabs(field);
        if (better(key, (int)pix, best.key, best.idx)) best = {key, (int)pix};
        if (weighted) {
            double w = win ? field * win[(size_t)s * plane + pix] : field;
            if (sens) w = sens[pix] * w;
            w = fabs(w);
            if (w > wbest) wbest = w;
        }
    }
    __shared__ Best s_best[kThreads / 64];
    __shared__ double s_w[kThreads / 64];
    best = wave_best(best);
    wbest = wave_max(wbest);
    if ((threadIdx.x & 63) == 0) {
        s_best[threadIdx.x >> 6] = best;
        s_w[threadIdx.x >> 6] = wbest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) {
            if (better(s_best[w].key, s_best[w].idx, best.key, best.idx)) best = s_best[w];
            if (s_w[w] > wbest) wbest = s_w[w];
        }
        const size_t t = ((size_t)s * p.nty + ty) * p.ntx + tx;
        tkey[t] = best.key;
        tidx[t] = best.idx;
        twkey[t] = weighted ? wbest : best.key;
    }
}

__global__ __launch_bounds__(kSelThreads) void k_select(Params p, State *st,
                                                        const double *__restrict__ res,
                                                        const double *__restrict__ hess,
                                                        const double *__restrict__ tkey,
                                                        const int *__restrict__ tidx,
                                                        const double *__restrict__ twkey) {
    __shared__ Best s_wave[kSelThreads / 64];
    __shared__ double s_wmax[kSelThreads / 64];
    __shared__ Best s_scale[kMaxScales];
    __shared__ double s_weighted[kMaxScales];
    __shared__ int s_done;
    if (threadIdx.x == 0) s_done = st->done;
    __syncthreads();
    if (s_done) {
        if (threadIdx.x == 0) st->active = 0;
        return;
    }
    const int ntiles = p.ntx * p.nty;
    for (int s = 0; s < p.ns; ++s) {
        Best best{-1.0, INT_MAX};
        double wmax = -1.0;
        for (int t = threadIdx.x; t < ntiles; t += kSelThreads) {
            const double k = tkey[(size_t)s * ntiles + t];
            const int i = tidx[(size_t)s * ntiles + t];
            const double w = twkey[(size_t)s * ntiles + t];
            if (better(k, i, best.key, best.idx)) best = {k, i};
            if (w > wmax) wmax = w;
        }
        best = wave_best(best);
        wmax = wave_max(wmax);
        if ((threadIdx.x & 63) == 0) {
            s_wave[threadIdx.x >> 6] = best;
            s_wmax[threadIdx.x >> 6] = wmax;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kSelThreads / 64; ++w) {
                if (better(s_wave[w].key, s_wave[w].idx, best.key, best.idx)) best = s_wave[w];
                if (s_wmax[w] > wmax) wmax = s_wmax[w];
            }
            // numpy.argmax of an all-NaN plane is 0 as well
            if (best.idx == INT_MAX) best.idx = 0;
            s_scale[s] = best;
            s_weighted[s] = wmax;
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    // the strict '>' of cleaners.py:1151, starting from optimum = 0 at (0, 0, scale 0)
    double optimum = 0.0;
    int pix = 0, ms = 0;
    for (int s = 0; s < p.ns; ++s) {
        if (s_weighted[s] > optimum) {
            optimum = s_weighted[s];
            ms = s;
            pix = s_scale[s].idx;
        }
    }
    // mval = smpsol[mscale, :, peak]
    const size_t plane = (size_t)p.ny * p.nx;
    const double *ihs = hess + (size_t)ms * kHess + kMaxMoments * kMaxMoments;
    double r[kMaxMoments], mval[kMaxMoments];
#pragma unroll
    for (int t = 0; t < kMaxMoments; ++t)
        r[t] = t < p.nt ? res[((size_t)ms * p.nt + t) * plane + pix] : 0.0;
#pragma unroll
    for (int n = 0; n < kMaxMoments; ++n) {
        double acc = ihs[n] * r[0];
#pragma unroll
        for (int m = 1; m < kMaxMoments; ++m)
            if (m < p.nt) acc = acc + ihs[m * kMaxMoments + n] * r[m];
        mval[n] = n < p.nt ? acc : 0.0;
    }
    st->iter += 1;
    st->counts[ms] += 1;
#pragma unroll
    for (int n = 0; n < kMaxMoments; ++n) st->mval[n] = mval[n];
    // the stop test comes before the update, without msclean's 0.9 (cleaners.py:854-864)
    if (fabs(mval[0]) < p.absthresh) {
        st->done = 1;
        st->active = 0;
        st->reason = SDP_HIP_CLEAN_STOP_THRESHOLD;
        return;
    }
    st->peak_y = pix / p.nx;
    st->peak_x = pix - (pix / p.nx) * p.nx;
    st->peak_s = ms;
    st->active = 1;
}

template <int T>
void run(const Params &p, hipStream_t st, State *state, double *res, const double *psf,
         const double *win, const double *sens, const double *skern, const double *hess,
         double *model, double *tkey, int *tidx, double *twkey, int niter, State *host) {
    k_update<T><<<dim3(p.ntx, p.nty, p.ns), kThreads, 0, st>>>(p, 1, state, res, psf, win, sens, skern,
                                                              hess, model, tkey, tidx, twkey);
    SDP_HIP_CHECK(hipGetLastError());
    // tiles a patch of 2 * (n // 2) pixels can touch at any offset
    auto span = [](int half, int tile, int total) {
        return std::min(total, (2 * half + tile - 2) / tile + 1);
    };
    const dim3 ugrid(span(p.pnx / 2, kTileX, p.ntx), span(p.pny / 2, kTileY, p.nty), p.ns + T);
    for (int issued = 0; issued < niter && !host->done;) {
        const int n = std::min(kBatch, niter - issued);
        for (int i = 0; i < n; ++i) {
            k_select<<<1, kSelThreads, 0, st>>>(p, state, res, hess, tkey, tidx, twkey);
            k_update<T><<<ugrid, kThreads, 0, st>>>(p, 0, state, res, psf, win, sens, skern, hess,
                                                    model, tkey, tidx, twkey);
        }
        SDP_HIP_CHECK(hipGetLastError());
        issued += n;
        SDP_HIP_CHECK(hipMemcpyAsync(host, state, sizeof(State), hipMemcpyDeviceToHost, st));
        SDP_HIP_CHECK(hipStreamSynchronize(st));
    }
}

}  // namespace mfsclean
}  // namespace sdp

extern "C" {

int sdp_hip_mfsclean_plane(int nscales, int nmoment, int ny, int nx, int psf_ny, int psf_nx,
                           double *smresidual, double *m_model, const double *ssmmpsf,
                           const double *scale_kernels, int scale_extent, const double *windowstack,
                           const double *sensitivity, const double *hsmmpsf, const double *ihsmmpsf,
                           int findpeak, double gain, double absthresh, int niter, int *niter_done,
                           int *stop_reason, int *scale_counts, void *stream, char *errbuf,
                           size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::mfsclean;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(nscales >= 1 && nscales <= kMaxScales, "nscales must be 1..16");
        SDP_REQUIRE(nmoment >= 1 && nmoment <= kMaxMoments, "nmoment must be 1..4");
        SDP_REQUIRE(ny > 0 && nx > 0 && (int64_t)ny * nx < INT_MAX,
                    "image must be non-empty with fewer than 2^31 pixels");
        SDP_REQUIRE(psf_ny >= 2 && psf_nx >= 2, "psf must be at least 2 x 2");
        SDP_REQUIRE(niter > 0, "niter must be positive");
        SDP_REQUIRE(findpeak == SDP_HIP_MFSCLEAN_FINDPEAK_RASCIL ||
                        findpeak == SDP_HIP_MFSCLEAN_FINDPEAK_CASA,
                    "findpeak must be SDP_HIP_MFSCLEAN_FINDPEAK_RASCIL or _CASA");
        SDP_REQUIRE(smresidual && m_model && ssmmpsf && scale_kernels && hsmmpsf && ihsmmpsf &&
                        niter_done && stop_reason && scale_counts,
                    "null pointer argument");
        Params p{};
        p.ns = nscales;
        p.nt = nmoment;
        p.ny = ny;
        p.nx = nx;
        p.pny = psf_ny;
        p.pnx = psf_nx;
        p.ntx = (nx + kTileX - 1) / kTileX;
        p.nty = (ny + kTileY - 1) / kTileY;
        p.kext = std::max(scale_extent, 0);
        p.casa = findpeak == SDP_HIP_MFSCLEAN_FINDPEAK_CASA;
        p.gain = gain;
        p.absthresh = absthresh;

        // hs then ihs of every scale, each padded to [4][4]
        std::vector<double> hhost((size_t)nscales * kHess, 0.0);
        for (int s = 0; s < nscales; ++s)
            for (int m = 0; m < nmoment; ++m)
                for (int n = 0; n < nmoment; ++n) {
                    const size_t src = ((size_t)s * nmoment + m) * nmoment + n;
                    hhost[(size_t)s * kHess + m * kMaxMoments + n] = hsmmpsf[src];
                    hhost[(size_t)s * kHess + kMaxMoments * kMaxMoments + m * kMaxMoments + n] =
                        ihsmmpsf[src];
                }

        const hipStream_t st = as_stream(stream);
        const size_t ntiles = (size_t)nscales * p.ntx * p.nty;
        State *state = scratch<State>("mfsclean_state", 1);
        double *hess = scratch<double>("mfsclean_hessians", hhost.size());
        double *tkey = scratch<double>("mfsclean_tile_key", ntiles);
        double *twkey = scratch<double>("mfsclean_tile_wkey", ntiles);
        int *tidx = scratch<int>("mfsclean_tile_idx", ntiles);
        SDP_HIP_CHECK(hipMemsetAsync(state, 0, sizeof(State), st));
        // hhost outlives the copy: run() synchronises the stream before it returns
        SDP_HIP_CHECK(hipMemcpyAsync(hess, hhost.data(), hhost.size() * sizeof(double),
                                     hipMemcpyHostToDevice, st));
        State host{};
        auto go = [&](auto tag) {
            run<decltype(tag)::value>(p, st, state, smresidual, ssmmpsf, windowstack, sensitivity,
                                      scale_kernels, hess, m_model, tkey, tidx, twkey, niter, &host);
        };
        switch (nmoment) {
            case 1: go(std::integral_constant<int, 1>{}); break;
            case 2: go(std::integral_constant<int, 2>{}); break;
            case 3: go(std::integral_constant<int, 3>{}); break;
            default: go(std::integral_constant<int, 4>{}); break;
        }
        *niter_done = host.iter;
        *stop_reason = host.done ? host.reason : SDP_HIP_CLEAN_STOP_NITER;
        for (int s = 0; s < nscales; ++s) scale_counts[s] = host.counts[s];
    });
}

}  // extern "C"
