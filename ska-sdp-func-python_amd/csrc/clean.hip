// CLEAN minor cycles for gfx950: sdp_hip_clean_plane runs up to niter cycles
// of Hogbom or multi-scale CLEAN on one image plane without leaving the
// device, restating the loops of the reference's
//   hogbom               src/ska_sdp_func_python/image/cleaners.py:23-133
//   msclean              cleaners.py:279-470 (the minor cycle, :403-452)
//   find_max_abs_stack   cleaners.py:565-610
//   overlapIndices       cleaners.py:235-267
// (the msclean set-up -- scale stacks, FFT convolutions, coupling matrix,
// window stack -- is the Python layer's).
//
// A cycle is two plain stream-ordered kernels and no host round trip:
//   k_select  one workgroup reduces the cached per-tile maxima to the next
//             peak, writes the component (Hogbom) and the pre-update stop
//             tests (msclean) and leaves the peak in device memory;
//   k_update  a grid sized by the PSF box reads that peak, subtracts the PSF
//             patch from every scale of the residual, adds the scale kernel
//             to the component image (msclean), refreshes the cached maxima
//             of the tiles the patch touches and applies Hogbom's
//             post-subtract stop test.
// Tiles the patch does not touch keep their cached maxima, so with a bounded
// PSF a cycle costs O(patch), not O(image).  The host enqueues cycles in
// batches and reads the stop flag once per batch; kernels launched after the
// stop return at once.  There is no grid-wide barrier and no spinning: every
// dependency is the stream order of two kernels.
//
// All arithmetic is fp64 in the reference's order with fp contraction off in
// this file, so the Hogbom residual and components are numpy's bit for bit.
// The search is numpy.argmax: the first maximum in row-major order, hence
// every reduction level breaks ties on the lower flat index, and scales are
// compared with the reference's strict '>' (the lower scale wins a tie).
// NaN search values are never selected.
//
// sdp_hip_clean_plane_complex is the same scheme for the reference's
//   hogbom_complex       cleaners.py:136-232
// on a Q and a U plane cleaned as P = Q + iU (k_select_c / k_update_c below).
#include "sdp_common.h"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace sdp {
namespace clean {

constexpr int kThreads = 256;
constexpr int kTileX = 64;  // one wave reads one 512-byte row segment
constexpr int kTileY = 16;
constexpr int kSelThreads = 1024;
constexpr int kMaxScales = 16;
constexpr int kBatch = 32;  // cycles enqueued between two reads of the stop flag

struct State {
    int done;    // stop decided (either kernel); k_select turns it into !active
    int active;  // written by k_select only: the next k_update has work
    int iter;    // cycles counted as the reference counts them
    int reason;  // SDP_HIP_CLEAN_STOP_*
    int peak_y, peak_x, peak_s, pad;
    double mval;
};

struct Params {
    int msclean, ns, ny, nx, pny, pnx;
    int ntx, nty;  // tiles per image plane
    int kext;      // scale kernels vanish beyond this many pixels from the PSF origin (0: unknown)
    double gain, pmax, thresh09;
    double coupling[kMaxScales];
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

// find_max_abs_stack's per-pixel values: `cmp` is |resid| after one
// multiplication by the sensitivity, the returned search key |resid * sens|
// has two (cleaners.py:593-603); Hogbom searches |res * window|.
__device__ __forceinline__ double search_key(const Params &p, int s, size_t pix, double v,
                                             const double *__restrict__ win,
                                             const double *__restrict__ sens, double *cmp) {
    double a = win ? v * win[(size_t)s * p.ny * p.nx + pix] : v;
    if (p.msclean) a = a / p.coupling[s];
    double key = a;
    if (sens) {
        a = a * sens[pix];
        key = a * sens[pix];
    }
    if (cmp) *cmp = fabs(a);
    return fabs(key);
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

// blockIdx.z < ns: residual scale z.  blockIdx.z == ns (msclean only): the
// component image.  init: every tile of the image, no subtraction.
__global__ __launch_bounds__(kThreads) void k_update(Params p, int init, State *st, double *res,
                                                     const double *__restrict__ psf,
                                                     const double *__restrict__ win,
                                                     const double *__restrict__ sens,
                                                     const double *__restrict__ skern,
                                                     double *comps, double *tkey, int *tidx) {
    int ty = blockIdx.y, tx = blockIdx.x;
    int py = 0, px = 0, ms = 0;
    double mval = 0.0;
    Box b{0, 0, 0, 0};
    if (!init) {
        if (!st->active) return;
        py = st->peak_y;
        px = st->peak_x;
        ms = st->peak_s;
        mval = st->mval;
        b = patch_box(p, py, px);
        if (blockIdx.z == p.ns && p.kext > 0)  // the component slice visits the kernel's support only
            b = {max(b.y0, py - p.kext), min(b.y1, py + p.kext + 1), max(b.x0, px - p.kext),
                 min(b.x1, px + p.kext + 1)};
        ty += b.y0 / kTileY;
        tx += b.x0 / kTileX;
        if (ty > (b.y1 - 1) / kTileY || tx > (b.x1 - 1) / kTileX) return;
    }
    const int s = blockIdx.z;
    const int hy = p.pny / 2, hx = p.pnx / 2;
    const size_t plane = (size_t)p.ny * p.nx, pplane = (size_t)p.pny * p.pnx;
    const int x = tx * kTileX + (threadIdx.x & 63);
    Best best{-1.0, INT_MAX};
#pragma unroll
    for (int k = 0; k < kTileY / 4; ++k) {
        const int y = ty * kTileY + (threadIdx.x >> 6) + 4 * k;
        if (y >= p.ny || x >= p.nx) continue;
        const size_t pix = (size_t)y * p.nx + x;
        const bool inbox = y >= b.y0 && y < b.y1 && x >= b.x0 && x < b.x1;
        const size_t ppix = inbox ? (size_t)(hy + y - py) * p.pnx + (hx + x - px) : 0;
        if (s == p.ns) {
            // comps[patch] += scale kernel * gain * mval (cleaners.py:446-450)
            if (inbox) comps[pix] = comps[pix] + skern[(size_t)ms * pplane + ppix] * p.gain * mval;
            continue;
        }
        double v = res[s * plane + pix];
        if (inbox) {
            const double t = psf[((size_t)s * p.ns + ms) * pplane + ppix];
            v = p.msclean ? v - t * p.gain * mval : v - t * mval;
            res[s * plane + pix] = v;
            // hogbom's stop test, after the subtraction (cleaners.py:109)
            if (!p.msclean && y == py && x == px && fabs(v) < p.thresh09) {
                st->done = 1;
                st->reason = SDP_HIP_CLEAN_STOP_THRESHOLD;
            }
        }
        const double key = search_key(p, s, pix, v, win, sens, nullptr);
        if (better(key, (int)pix, best.key, best.idx)) best = {key, (int)pix};
    }
    if (s == p.ns) return;
    __shared__ Best s_best[kThreads / 64];
    best = wave_best(best);
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w)
            if (better(s_best[w].key, s_best[w].idx, best.key, best.idx)) best = s_best[w];
        const size_t t = ((size_t)s * p.nty + ty) * p.ntx + tx;
        tkey[t] = best.key;
        tidx[t] = best.idx;
    }
}

__global__ __launch_bounds__(kSelThreads) void k_select(Params p, State *st,
                                                        const double *__restrict__ res,
                                                        const double *__restrict__ win,
                                                        const double *__restrict__ sens,
                                                        double *comps,
                                                        const double *__restrict__ tkey,
                                                        const int *__restrict__ tidx) {
    __shared__ Best s_wave[kSelThreads / 64];
    __shared__ Best s_scale[kMaxScales];
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
        for (int t = threadIdx.x; t < ntiles; t += kSelThreads) {
            const double k = tkey[(size_t)s * ntiles + t];
            const int i = tidx[(size_t)s * ntiles + t];
            if (better(k, i, best.key, best.idx)) best = {k, i};
        }
        best = wave_best(best);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kSelThreads / 64; ++w)
                if (better(s_wave[w].key, s_wave[w].idx, best.key, best.idx)) best = s_wave[w];
            // numpy.argmax of an all-NaN plane is 0 as well
            if (best.idx == INT_MAX) best.idx = 0;
            s_scale[s] = best;
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const size_t plane = (size_t)p.ny * p.nx;
    int pix = s_scale[0].idx, ms = 0;
    if (p.msclean) {
        // the strict '>' of cleaners.py:604, starting from pabsmax = 0 at (0, 0, 0)
        double pabsmax = 0.0;
        pix = 0;
        for (int s = 0; s < p.ns; ++s) {
            double cmp;
            const int i = s_scale[s].idx;
            search_key(p, s, (size_t)i, res[s * plane + i], win, sens, &cmp);
            if (cmp > pabsmax) {
                pabsmax = cmp;
                pix = i;
                ms = s;
            }
        }
    }
    const double r = res[ms * plane + pix];
    double mval;
    st->iter += 1;
    if (p.msclean) {
        mval = r / p.coupling[ms];
        if (fabs(r) < p.thresh09 || !(fabs(mval) > 0.0)) {
            st->done = 1;
            st->active = 0;
            st->reason = fabs(r) < p.thresh09 ? SDP_HIP_CLEAN_STOP_THRESHOLD : SDP_HIP_CLEAN_STOP_ZERO;
            return;
        }
    } else {
        mval = r * p.gain / p.pmax;
        comps[pix] = comps[pix] + mval;
    }
    st->peak_y = pix / p.nx;
    st->peak_x = pix - (pix / p.nx) * p.nx;
    st->peak_s = ms;
    st->mval = mval;
    st->active = 1;
}

// ---- complex Hogbom: Q and U cleaned together as P = Q + iU ------------------
// (hogbom_complex, cleaners.py:136-232).  The same two kernels per cycle on a
// residual of two planes: the search key of a pixel is hypot(q * w, u * w), one
// thread owns the pixel in both planes and reads its PSF value once.  Params
// carries the geometry and the gain (ns 1, msclean 0); 1 / pmax and the
// threshold, which is not scaled by 0.9 here, are kernel arguments.
struct StateC {
    int done, active, iter, reason;  // as State
    int peak_y, peak_x;
    double mval_q, mval_u;
};

__device__ __forceinline__ double key_c(double q, double u, size_t pix,
                                        const double *__restrict__ win) {
    return win ? hypot(q * win[pix], u * win[pix]) : hypot(q, u);
}

// init: every tile of the image, no subtraction.
__global__ __launch_bounds__(kThreads) void k_update_c(Params p, double absthresh, int init,
                                                       StateC *st, double *res,
                                                       const double *__restrict__ psf,
                                                       const double *__restrict__ win,
                                                       double *tkey, int *tidx) {
    int ty = blockIdx.y, tx = blockIdx.x;
    int py = 0, px = 0;
    double mq = 0.0, mu = 0.0;
    Box b{0, 0, 0, 0};
    if (!init) {
        if (!st->active) return;
        py = st->peak_y;
        px = st->peak_x;
        mq = st->mval_q;
        mu = st->mval_u;
        b = patch_box(p, py, px);
        ty += b.y0 / kTileY;
        tx += b.x0 / kTileX;
        if (ty > (b.y1 - 1) / kTileY || tx > (b.x1 - 1) / kTileX) return;
    }
    const int hy = p.pny / 2, hx = p.pnx / 2;
    const size_t plane = (size_t)p.ny * p.nx;
    const int x = tx * kTileX + (threadIdx.x & 63);
    Best best{-1.0, INT_MAX};
#pragma unroll
    for (int k = 0; k < kTileY / 4; ++k) {
        const int y = ty * kTileY + (threadIdx.x >> 6) + 4 * k;
        if (y >= p.ny || x >= p.nx) continue;
        const size_t pix = (size_t)y * p.nx + x;
        double q = res[pix], u = res[plane + pix];
        if (y >= b.y0 && y < b.y1 && x >= b.x0 && x < b.x1) {
            const double t = psf[(size_t)(hy + y - py) * p.pnx + (hx + x - px)];
            q = q - t * mq;
            u = u - t * mu;
            res[pix] = q;
            res[plane + pix] = u;
            // the stop test, after the subtraction and on absthresh itself (cleaners.py:222)
            if (y == py && x == px && hypot(q, u) < absthresh) {
                st->done = 1;
                st->reason = SDP_HIP_CLEAN_STOP_THRESHOLD;
            }
        }
        const double key = key_c(q, u, pix, win);
        if (better(key, (int)pix, best.key, best.idx)) best = {key, (int)pix};
    }
    __shared__ Best s_best[kThreads / 64];
    best = wave_best(best);
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w)
            if (better(s_best[w].key, s_best[w].idx, best.key, best.idx)) best = s_best[w];
        const size_t t = (size_t)ty * p.ntx + tx;
        tkey[t] = best.key;
        tidx[t] = best.idx;
    }
}

__global__ __launch_bounds__(kSelThreads) void k_select_c(Params p, double rinv, StateC *st,
                                                          const double *__restrict__ res,
                                                          double *comps,
                                                          const double *__restrict__ tkey,
                                                          const int *__restrict__ tidx) {
    __shared__ Best s_wave[kSelThreads / 64];
    __shared__ int s_done;
    if (threadIdx.x == 0) s_done = st->done;
    __syncthreads();
    if (s_done) {
        if (threadIdx.x == 0) st->active = 0;
        return;
    }
    const int ntiles = p.ntx * p.nty;
    Best best{-1.0, INT_MAX};
    for (int t = threadIdx.x; t < ntiles; t += kSelThreads)
        if (better(tkey[t], tidx[t], best.key, best.idx)) best = {tkey[t], tidx[t]};
    best = wave_best(best);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kSelThreads / 64; ++w)
        if (better(s_wave[w].key, s_wave[w].idx, best.key, best.idx)) best = s_wave[w];
    // numpy.argmax of an all-NaN plane is 0 as well
    const int pix = best.idx == INT_MAX ? 0 : best.idx;
    const size_t plane = (size_t)p.ny * p.nx;
    // numpy's complex / real: one reciprocal, then a product per component
    const double mq = (res[pix] * p.gain) * rinv;
    const double mu = (res[plane + pix] * p.gain) * rinv;
    comps[pix] = comps[pix] + mq;
    comps[plane + pix] = comps[plane + pix] + mu;
    st->iter += 1;
    st->peak_y = pix / p.nx;
    st->peak_x = pix - (pix / p.nx) * p.nx;
    st->mval_q = mq;
    st->mval_u = mu;
    st->active = 1;
}

}  // namespace clean
}  // namespace sdp

extern "C" {

int sdp_hip_clean_plane(int algorithm, int nscales, int ny, int nx, int psf_ny, int psf_nx,
                        double *res, const double *psf, const double *window,
                        const double *sensitivity, const double *coupling_diag,
                        const double *scale_kernels, int scale_extent, double *comps, double gain,
                        double pmax, double absthresh, int niter, int *niter_done, int *stop_reason,
                        void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::clean;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(algorithm == SDP_HIP_CLEAN_HOGBOM || algorithm == SDP_HIP_CLEAN_MSCLEAN,
                    "algorithm must be SDP_HIP_CLEAN_HOGBOM or SDP_HIP_CLEAN_MSCLEAN");
        const bool ms = algorithm == SDP_HIP_CLEAN_MSCLEAN;
        SDP_REQUIRE(nscales >= 1 && nscales <= kMaxScales, "nscales must be 1..16");
        SDP_REQUIRE(ms || nscales == 1, "hogbom takes one scale");
        SDP_REQUIRE(ny > 0 && nx > 0 && (int64_t)ny * nx < INT_MAX,
                    "image must be non-empty with fewer than 2^31 pixels");
        SDP_REQUIRE(psf_ny >= 2 && psf_nx >= 2, "psf must be at least 2 x 2");
        SDP_REQUIRE(niter > 0, "niter must be positive");
        SDP_REQUIRE(res && psf && comps && niter_done && stop_reason, "null pointer argument");
        SDP_REQUIRE(!ms || (coupling_diag && scale_kernels),
                    "msclean needs coupling_diag and scale_kernels");
        SDP_REQUIRE(ms || !sensitivity, "hogbom takes no sensitivity");
        Params p{};
        p.msclean = ms;
        p.ns = nscales;
        p.ny = ny;
        p.nx = nx;
        p.pny = psf_ny;
        p.pnx = psf_nx;
        p.ntx = (nx + kTileX - 1) / kTileX;
        p.nty = (ny + kTileY - 1) / kTileY;
        p.gain = gain;
        p.pmax = pmax;
        p.thresh09 = 0.9 * absthresh;
        p.kext = std::max(scale_extent, 0);
        for (int s = 0; s < nscales; ++s) p.coupling[s] = ms ? coupling_diag[s] : 1.0;

        const hipStream_t st = as_stream(stream);
        const size_t ntiles = (size_t)nscales * p.ntx * p.nty;
        State *state = scratch<State>("clean_state", 1);
        double *tkey = scratch<double>("clean_tile_key", ntiles);
        int *tidx = scratch<int>("clean_tile_idx", ntiles);
        SDP_HIP_CHECK(hipMemsetAsync(state, 0, sizeof(State), st));
        k_update<<<dim3(p.ntx, p.nty, nscales), kThreads, 0, st>>>(
            p, 1, state, res, psf, window, sensitivity, scale_kernels, comps, tkey, tidx);
        SDP_HIP_CHECK(hipGetLastError());

        // tiles a patch of 2 * (n // 2) pixels can touch at any offset
        auto span = [](int half, int tile, int total) {
            return std::min(total, (2 * half + tile - 2) / tile + 1);
        };
        const dim3 ugrid(span(psf_nx / 2, kTileX, p.ntx), span(psf_ny / 2, kTileY, p.nty),
                         nscales + (ms ? 1 : 0));
        State host{};
        for (int issued = 0; issued < niter && !host.done;) {
            const int n = std::min(kBatch, niter - issued);
            for (int i = 0; i < n; ++i) {
                k_select<<<1, kSelThreads, 0, st>>>(p, state, res, window, sensitivity, comps, tkey, tidx);
                k_update<<<ugrid, kThreads, 0, st>>>(p, 0, state, res, psf, window, sensitivity,
                                                     scale_kernels, comps, tkey, tidx);
            }
            SDP_HIP_CHECK(hipGetLastError());
            issued += n;
            SDP_HIP_CHECK(hipMemcpyAsync(&host, state, sizeof(State), hipMemcpyDeviceToHost, st));
            SDP_HIP_CHECK(hipStreamSynchronize(st));
        }
        *niter_done = host.iter;
        *stop_reason = host.done ? host.reason : SDP_HIP_CLEAN_STOP_NITER;
    });
}

int sdp_hip_clean_plane_complex(int ny, int nx, int psf_ny, int psf_nx, double *res,
                                const double *psf, const double *window, double *comps,
                                double gain, double pmax, double absthresh, int niter,
                                int *niter_done, int *stop_reason, void *stream, char *errbuf,
                                size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::clean;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(ny > 0 && nx > 0 && (int64_t)ny * nx < INT_MAX,
                    "image must be non-empty with fewer than 2^31 pixels");
        SDP_REQUIRE(psf_ny >= 2 && psf_nx >= 2, "psf must be at least 2 x 2");
        SDP_REQUIRE(niter > 0, "niter must be positive");
        SDP_REQUIRE(pmax > 0.0, "pmax must be positive");
        SDP_REQUIRE(res && psf && comps && niter_done && stop_reason, "null pointer argument");
        Params p{};
        p.ns = 1;
        p.ny = ny;
        p.nx = nx;
        p.pny = psf_ny;
        p.pnx = psf_nx;
        p.ntx = (nx + kTileX - 1) / kTileX;
        p.nty = (ny + kTileY - 1) / kTileY;
        p.gain = gain;
        p.pmax = pmax;
        const double rinv = 1.0 / pmax;

        const hipStream_t st = as_stream(stream);
        const size_t ntiles = (size_t)p.ntx * p.nty;
        StateC *state = scratch<StateC>("clean_complex_state", 1);
        double *tkey = scratch<double>("clean_complex_tile_key", ntiles);
        int *tidx = scratch<int>("clean_complex_tile_idx", ntiles);
        SDP_HIP_CHECK(hipMemsetAsync(state, 0, sizeof(StateC), st));
        k_update_c<<<dim3(p.ntx, p.nty), kThreads, 0, st>>>(p, absthresh, 1, state, res, psf,
                                                            window, tkey, tidx);
        SDP_HIP_CHECK(hipGetLastError());

        // tiles a patch of 2 * (n // 2) pixels can touch at any offset
        auto span = [](int half, int tile, int total) {
            return std::min(total, (2 * half + tile - 2) / tile + 1);
        };
        const dim3 ugrid(span(psf_nx / 2, kTileX, p.ntx), span(psf_ny / 2, kTileY, p.nty));
        StateC host{};
        for (int issued = 0; issued < niter && !host.done;) {
            const int n = std::min(kBatch, niter - issued);
            for (int i = 0; i < n; ++i) {
                k_select_c<<<1, kSelThreads, 0, st>>>(p, rinv, state, res, comps, tkey, tidx);
                k_update_c<<<ugrid, kThreads, 0, st>>>(p, absthresh, 0, state, res, psf, window,
                                                       tkey, tidx);
            }
            SDP_HIP_CHECK(hipGetLastError());
            issued += n;
            SDP_HIP_CHECK(hipMemcpyAsync(&host, state, sizeof(StateC), hipMemcpyDeviceToHost, st));
            SDP_HIP_CHECK(hipStreamSynchronize(st));
        }
        *niter_done = host.iter;
        *stop_reason = host.done ? host.reason : SDP_HIP_CLEAN_STOP_NITER;
    });
}

}  // extern "C"
