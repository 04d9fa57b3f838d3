// Oversampled w-projection kernels for gfx950: sdp_hip_wkernel_create
// (include/ska_sdp_hip.h), behind grid_data/convolution_functions.py.
//
// The recipe it serves is w_beam -> taper -> pad_mid to os * N -> centred
// inverse FFT -> extract_oversampled for every sub-grid offset.  Of the padded
// transform only J = nd * support samples per axis are ever read
// (j = os * (k - support / 2) - s for the kernel pixel k and the signed offset
// s in [-h, h]) and only N of its os * N input rows and columns are non-zero,
// so each plane is two small complex matrix products
//     T = A E^T           [N x J]     T[y][jx] = sum_x A[y][x] E[jx][x]
//     F = E T / N^2       [J x J]     F[jy][jx] = sum_y E[jy][y] T[y][jx]
// with E[j][x] = exp(2 pi i ((j (x - N / 2)) mod Npad) / Npad), and F lands in
// the convolution function's layout [iv][iu][kv][ku] directly.
//
//   k_twiddle   E [J x N], once per call: the exponent is reduced as an
//               integer to (-Npad / 2, Npad / 2] and handed to sincospi.
//   k_farfield  A for a chunk of planes: the w beam by the reference's own
//               expression -2 pi w (1 - sqrt(1 - r2)), cancellation included
//               (every operation rounded once: fp contraction is off in this
//               file), times the separable taper, times the primary beam.
//   k_cgemm     both products: 64 x 64 output tile per workgroup of 256, a 4 x 4
//               block of complex sums per thread, K staged through LDS 16 at a
//               time, plain fp64 FMAs.  Every sum runs over ascending k from
//               +0 with the same four FMAs per term whatever the position of
//               its element in a tile (tile edges are zero-filled, and adding
//               +0 products changes nothing), so an element's bits depend on
//               its operands alone.  No atomics.
#include "sdp_common.h"

#pragma clang fp contract(off)

namespace sdp {
namespace wkernel {

constexpr int kThreads = 256;
constexpr int kTile = 64;    // output tile edge
constexpr int kTileK = 16;   // K per LDS stage
constexpr int kPad = 1;      // one 16-byte slot per LDS row against bank conflicts
constexpr int kMaxPixel = 4096;
constexpr int kMaxSamples = 32768;
constexpr size_t kChunkBytes = (size_t)256 << 20;  // far fields + T held at a time
constexpr int kMaxChunk = 32768;                   // planes per launch (gridDim.z)

// row r of E belongs to offset plane i = r / support and kernel pixel
// k = r % support
__device__ __forceinline__ int sample_of_row(int r, int os, int support) {
    const int i = r / support, k = r - i * support;
    return os * (k - support / 2) - (i - os / 2);
}

__global__ __launch_bounds__(kThreads) void k_twiddle(double2 *__restrict__ e, int nsamp, int n,
                                                      int os, int support) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)nsamp * n) return;
    const int r = (int)(idx / n), x = (int)(idx - (int64_t)r * n);
    const int64_t npad = (int64_t)os * n;
    int64_t m = ((int64_t)sample_of_row(r, os, support) * (x - n / 2)) % npad;
    if (m < 0) m += npad;
    if (2 * m > npad) m -= npad;
    double s, c;
    sincospi(2.0 * (double)m / (double)npad, &s, &c);
    e[idx] = make_double2(c, s);
}

// planes p0 .. p0 + np - 1 of the call's npb * nw; plane p has w[p % nw] and
// pb[p / nw]
__global__ __launch_bounds__(kThreads) void k_farfield(double2 *__restrict__ a, int n, int64_t p0,
                                                       int np, int nw, double fov,
                                                       const double *__restrict__ w,
                                                       const double *__restrict__ taper,
                                                       const double2 *__restrict__ pb) {
    const int64_t nn = (int64_t)n * n;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= nn * np) return;
    const int64_t p = p0 + idx / nn;
    const int64_t pix = idx % nn;
    const int y = (int)(pix / n), x = (int)(pix - (int64_t)y * n);
    const double ly = (double)(y - n / 2) / (double)n;
    const double mx = (double)(x - n / 2) / (double)n;
    const double r2 = (fov * fov) * (ly * ly + mx * mx);
    // the reference's w_beam(npixel, fov, -w): ph = -2 pi (-w) (1 - sqrt(1 - r2))
    const double wz = -w[p % nw];
    double re = 0.0, im = 0.0;
    if (r2 == 0.0) {
        re = 1.0;
    } else if (r2 < 1.0) {
        const double ph = ((-2.0 * M_PI) * wz) * (1.0 - sqrt(1.0 - r2));
        sincos(ph, &im, &re);
    }
    if (taper) {
        const double tt = taper[y] * taper[x];
        re = re * tt;
        im = im * tt;
    }
    if (pb) {
        const double2 b = pb[(p / nw) * nn + pix];
        const double r = re * b.x - im * b.y;
        im = re * b.y + im * b.x;
        re = r;
    }
    a[idx] = make_double2(re, im);
}

// C[m][n] = sum_k A[m][k] * B(k, n) for plane blockIdx.z.
//   SECOND == false:  A = far field of the plane [M = npix][K = npix], B(k, n) =
//                     e[n][k]; C = T of the plane [npix][nsamp], stored as is.
//   SECOND == true:   A = e [M = nsamp][K = npix] (shared by all planes), B(k, n)
//                     = T[k][n]; C / npix^2 goes to cf[iv][iu][kv][ku] with
//                     m = iv * support + kv, n = iu * support + ku.
template <bool SECOND>
__global__ __launch_bounds__(kThreads) void k_cgemm(const double2 *__restrict__ far,
                                                    const double2 *__restrict__ e,
                                                    double2 *__restrict__ t,
                                                    double2 *__restrict__ cf, int npix, int nsamp,
                                                    int support, int nd) {
    __shared__ double2 as[kTileK][kTile + kPad];
    __shared__ double2 bs[kTileK][kTile + kPad];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * kTile, m0 = blockIdx.y * kTile;
    const int64_t plane = blockIdx.z;
    const int M = SECOND ? nsamp : npix, K = npix, N = nsamp;
    const double2 *A = SECOND ? e : far + plane * (int64_t)npix * npix;
    const double2 *T = t + plane * (int64_t)npix * nsamp;
    const double2 zero = make_double2(0.0, 0.0);

    double cr[4][4], ci[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) cr[i][j] = ci[i][j] = 0.0;

    for (int k0 = 0; k0 < K; k0 += kTileK) {
        // A (and stage 1's B) have k contiguous: 16 lanes along k, 16 rows a pass
        const int lk = tid & 15, lr = tid >> 4;
#pragma unroll
        for (int pass = 0; pass < kTile / 16; ++pass) {
            const int r = pass * 16 + lr;
            const bool kin = k0 + lk < K;
            as[lk][r] = (kin && m0 + r < M) ? A[(int64_t)(m0 + r) * K + k0 + lk] : zero;
            if (!SECOND)
                bs[lk][r] = (kin && n0 + r < N) ? e[(int64_t)(n0 + r) * K + k0 + lk] : zero;
        }
        if (SECOND) {
            // T has n contiguous: 64 lanes along n, 4 values of k a pass
            const int ln = tid & 63, lkk = tid >> 6;
#pragma unroll
            for (int pass = 0; pass < kTileK / 4; ++pass) {
                const int k = pass * 4 + lkk;
                bs[k][ln] = (k0 + k < K && n0 + ln < N) ? T[(int64_t)(k0 + k) * N + n0 + ln] : zero;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kTileK; ++k) {
            double2 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = as[k][ty * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = bs[k][tx * 4 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cr[i][j] = fma(a[i].x, b[j].x, cr[i][j]);
                    cr[i][j] = fma(-a[i].y, b[j].y, cr[i][j]);
                    ci[i][j] = fma(a[i].x, b[j].y, ci[i][j]);
                    ci[i][j] = fma(a[i].y, b[j].x, ci[i][j]);
                }
        }
        __syncthreads();
    }

    if (!SECOND) {
        double2 *C = t + plane * (int64_t)npix * nsamp;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + ty * 4 + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + tx * 4 + j;
                if (m < M && n < N) C[(int64_t)m * N + n] = make_double2(cr[i][j], ci[i][j]);
            }
        }
    } else {
        double2 *C = cf + plane * (int64_t)nsamp * nsamp;
        const double div = (double)npix * (double)npix;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + ty * 4 + i;
            const int iv = m / support, kv = m - iv * support;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + tx * 4 + j;
                const int iu = n / support, ku = n - iu * support;
                if (m < M && n < N)
                    C[(((int64_t)iv * nd + iu) * support + kv) * support + ku] =
                        make_double2(cr[i][j] / div, ci[i][j] / div);
            }
        }
    }
}

}  // namespace wkernel
}  // namespace sdp

extern "C" {

int sdp_hip_wkernel_create(int npixel, int oversampling, int support, int nw, int npb,
                           double field_of_view, const double *w, const double *taper,
                           const void *pb, void *cf, void *stream, char *errbuf,
                           size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::wkernel;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(support >= 2 && support % 2 == 0, "wkernel: support must be even and >= 2");
        SDP_REQUIRE(npixel % 2 == 0 && npixel >= support + 2 && npixel <= kMaxPixel,
                    "wkernel: npixel must be even, >= support + 2 and <= " +
                        std::to_string(kMaxPixel));
        SDP_REQUIRE(oversampling >= 1, "wkernel: oversampling must be >= 1");
        const int64_t nd = 2 * (int64_t)(oversampling / 2) + 1;
        SDP_REQUIRE(nd * support <= kMaxSamples,
                    "wkernel: (2 (oversampling / 2) + 1) * support must be <= " +
                        std::to_string(kMaxSamples));
        SDP_REQUIRE(nw >= 1 && npb >= 1 && (int64_t)nw * npb < ((int64_t)1 << 31),
                    "wkernel: nw and npb must be >= 1 and nw * npb < 2^31");
        SDP_REQUIRE(pb || npb == 1, "wkernel: npb must be 1 without a primary beam");
        SDP_REQUIRE(field_of_view == field_of_view, "wkernel: field_of_view is NaN");
        SDP_REQUIRE(w && cf, "null pointer argument");
        SDP_REQUIRE(reinterpret_cast<uintptr_t>(w) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(taper) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(pb) % 16 == 0 &&
                        reinterpret_cast<uintptr_t>(cf) % 16 == 0,
                    "wkernel: a pointer is not aligned to its element");

        const int nsamp = (int)(nd * support);
        const int64_t planes = (int64_t)nw * npb;
        const size_t per_plane = sizeof(double2) * ((size_t)npixel * npixel + (size_t)npixel * nsamp);
        const int chunk = (int)std::min<int64_t>(
            planes, std::max<int64_t>(1, std::min<int64_t>(kMaxChunk, (int64_t)(kChunkBytes / per_plane))));
        const hipStream_t st = as_stream(stream);

        double2 *e = scratch<double2>("wkernel_twiddle", (size_t)nsamp * npixel);
        double2 *far = scratch<double2>("wkernel_far", (size_t)chunk * npixel * npixel);
        double2 *t = scratch<double2>("wkernel_t", (size_t)chunk * npixel * nsamp);
        k_twiddle<<<grid1d((int64_t)nsamp * npixel, kThreads), kThreads, 0, st>>>(
            e, nsamp, npixel, oversampling, support);
        SDP_HIP_CHECK(hipGetLastError());

        const unsigned gs = (unsigned)((nsamp + kTile - 1) / kTile);
        const unsigned gp = (unsigned)((npixel + kTile - 1) / kTile);
        for (int64_t p0 = 0; p0 < planes; p0 += chunk) {
            const int np = (int)std::min<int64_t>(chunk, planes - p0);
            k_farfield<<<grid1d((int64_t)np * npixel * npixel, kThreads), kThreads, 0, st>>>(
                far, npixel, p0, np, nw, field_of_view, w, taper, static_cast<const double2 *>(pb));
            SDP_HIP_CHECK(hipGetLastError());
            k_cgemm<false><<<dim3(gs, gp, (unsigned)np), kThreads, 0, st>>>(
                far, e, t, nullptr, npixel, nsamp, support, (int)nd);
            SDP_HIP_CHECK(hipGetLastError());
            k_cgemm<true><<<dim3(gs, gs, (unsigned)np), kThreads, 0, st>>>(
                nullptr, e, t, static_cast<double2 *>(cf) + p0 * (int64_t)nsamp * nsamp, npixel,
                nsamp, support, (int)nd);
            SDP_HIP_CHECK(hipGetLastError());
        }
    });
}

}  // extern "C"
