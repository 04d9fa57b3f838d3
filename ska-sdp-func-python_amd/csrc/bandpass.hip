// Bandpass resampling for gfx950 (reference src/ska_sdp_func_python/
// calibration/beamformer_utils.py:273-491): the gain spectra of a table
// [rows][c_in][R][R] complex128 re-channelised onto c_out output channels.
//
//   sdp_hip_resample_polyfit   least-squares polynomial per segment of the band
//   sdp_hip_resample_interp    numpy.interp on complex data, bit for bit
//
// Every spectrum of a table shares its abscissae and none carries weights, so
// the polynomial fit is one linear operator along the channel axis.  The host
// hands it over factored through polynomials orthonormal on each segment's
// input channels: Q[d][c] (values at the input channels) and E[co][d] (values
// at the output channels), so that the fitted value is
//   out[co] = sum_d E[co][d] * (sum_c Q[d][c] g[c])     c in segment seg[co].
//
// k_polyfit: one workgroup of 256 lanes per row.  Per segment the lanes stride
// over the input channels; a lane reads a whole R x R group (64 contiguous
// bytes for R = 2, so a wavefront reads 4 KiB in one piece) and adds Q[d][c] *
// g[c][r] into (degree + 1) x 2 R R registers.  The partial sums are combined
// by an xor butterfly within each wavefront (both partners of a step add the
// same two numbers, so all 64 lanes hold the same bits), then lane 0 of every
// wavefront stores them to LDS and the first lanes add the four wavefronts'
// values in ascending order.  The coefficients of all segments stay in LDS;
// the lanes then stride over the output channels.  Nothing is atomic and the
// workgroup shape never depends on the batch, so a row's bits depend on that
// row alone.  fp64 throughout, contraction off.
//
// k_interp: one lane per (row, output channel), the interval index found on
// the host.  The arithmetic is that of numpy's arr_interp_complex: the slope
// is (y[j+1] - y[j]) * (1 / (x[j+1] - x[j])) per component, the value
// slope * (x - x[j]) + y[j], with numpy's two NaN fallbacks.
#include "sdp_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace sdp {
namespace bandpass {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDegree = SDP_HIP_BANDPASS_MAX_DEGREE;
constexpr int kMaxSegments = SDP_HIP_BANDPASS_MAX_SEGMENTS;
constexpr int kInterpBlocks = 1 << 16;  // (row, channel) pairs beyond that: grid-stride loop

// NC doubles (one R x R group of complex128) from / to 16-byte aligned memory
template <int NC>
__device__ __forceinline__ void load_group(const double *p, double (&v)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; k += 2) {
        const double2 t = *reinterpret_cast<const double2 *>(p + k);
        v[k] = t.x;
        v[k + 1] = t.y;
    }
}

template <int NC>
__device__ __forceinline__ void store_group(double *p, const double (&v)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; k += 2) *reinterpret_cast<double2 *>(p + k) = make_double2(v[k], v[k + 1]);
}

template <int NC, int ND>
__global__ __launch_bounds__(kThreads) void k_polyfit(const double *__restrict__ gain,
                                                      double *__restrict__ out,
                                                      const double *__restrict__ q,
                                                      const double *__restrict__ e,
                                                      const int32_t *__restrict__ seg,
                                                      const int32_t *__restrict__ edges, int nseg,
                                                      int c_in, int c_out) {
    constexpr int NV = ND * NC;
    extern __shared__ double lds[];
    double *coef = lds;              // [nseg][ND][NC]
    double *part = lds + nseg * NV;  // [kWaves][ND][NC]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *g = gain + (size_t)blockIdx.x * c_in * NC;

    for (int s = 0; s < nseg; ++s) {
        double acc[ND][NC];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < NC; ++r) acc[d][r] = 0.0;
        // the host checked 0 <= edges[s] <= edges[s + 1] <= c_in; clamped all the same
        const int c0 = max(edges[s], 0), c1 = min(edges[s + 1], c_in);
        for (int c = c0 + tid; c < c1; c += kThreads) {
            double v[NC];
            load_group<NC>(g + (size_t)c * NC, v);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const double qd = q[(size_t)d * c_in + c];
#pragma unroll
                for (int r = 0; r < NC; ++r) acc[d][r] = acc[d][r] + qd * v[r];
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < NC; ++r) {
                double a = acc[d][r];
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) a = a + __shfl_xor(a, o, 64);
                acc[d][r] = a;
            }
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < ND; ++d)
#pragma unroll
                for (int r = 0; r < NC; ++r) part[wave * NV + d * NC + r] = acc[d][r];
        }
        __syncthreads();
        if (tid < NV) {
            double t = part[tid];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) t = t + part[w * NV + tid];
            coef[s * NV + tid] = t;
        }
        __syncthreads();
    }

    double *o = out + (size_t)blockIdx.x * c_out * NC;
    for (int co = tid; co < c_out; co += kThreads) {
        const int s = seg[co];
        double v[NC];
        if (s < 0 || s >= nseg) {
#pragma unroll
            for (int r = 0; r < NC; ++r) v[r] = __builtin_nan("");
        } else {
            const double *cf = coef + s * NV;
            const double *ee = e + (size_t)co * ND;
            const double e0 = ee[0];
#pragma unroll
            for (int r = 0; r < NC; ++r) v[r] = e0 * cf[r];
#pragma unroll
            for (int d = 1; d < ND; ++d) {
                const double ed = ee[d];
#pragma unroll
                for (int r = 0; r < NC; ++r) v[r] = v[r] + ed * cf[d * NC + r];
            }
        }
        store_group<NC>(o + (size_t)co * NC, v);
    }
}

template <int NC>
__global__ __launch_bounds__(kThreads) void k_interp(const double *__restrict__ gain,
                                                     double *__restrict__ out,
                                                     const double *__restrict__ x_in,
                                                     const double *__restrict__ x_out,
                                                     const int32_t *__restrict__ interval,
                                                     int64_t nrows, int c_in, int c_out) {
    const int64_t total = nrows * c_out;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * kThreads) {
        const int64_t row = i / c_out;
        const int co = (int)(i - row * c_out);
        const double *g = gain + (size_t)row * c_in * NC;
        const int j = interval[co];
        const double x = x_out[co];
        double v[NC];
        if (j == -2) {  // a NaN abscissa: numpy returns x + 0j
#pragma unroll
            for (int k = 0; k < NC; k += 2) {
                v[k] = x;
                v[k + 1] = 0.0;
            }
        } else if (j < 0) {
            load_group<NC>(g, v);
        } else if (j >= c_in - 1) {
            load_group<NC>(g + (size_t)(c_in - 1) * NC, v);
        } else {
            const double x0 = x_in[j], x1 = x_in[j + 1];
            double y0[NC], y1[NC];
            load_group<NC>(g + (size_t)j * NC, y0);
            if (x0 == x) {
#pragma unroll
                for (int k = 0; k < NC; ++k) v[k] = y0[k];
            } else {
                load_group<NC>(g + (size_t)(j + 1) * NC, y1);
                const double inv_dx = 1.0 / (x1 - x0);
                const double dl = x - x0, dr = x - x1;
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const double slope = (y1[k] - y0[k]) * inv_dx;
                    double r = slope * dl + y0[k];
                    if (isnan(r)) {
                        r = slope * dr + y1[k];
                        if (isnan(r) && y0[k] == y1[k]) r = y0[k];
                    }
                    v[k] = r;
                }
            }
        }
        store_group<NC>(out + (size_t)i * NC, v);
    }
}

template <int NC, int ND>
void launch_polyfit(const double *gain, double *out, const double *q, const double *e,
                    const int32_t *seg, const int32_t *edges, int nseg, int64_t nrows, int c_in,
                    int c_out, hipStream_t st) {
    const size_t lds = (size_t)(nseg + kWaves) * ND * NC * sizeof(double);
    hipLaunchKernelGGL((k_polyfit<NC, ND>), dim3((unsigned)nrows), dim3(kThreads), lds, st, gain, out,
                       q, e, seg, edges, nseg, c_in, c_out);
    SDP_HIP_CHECK(hipGetLastError());
}

template <int NC>
void dispatch_polyfit(int nd, const double *gain, double *out, const double *q, const double *e,
                      const int32_t *seg, const int32_t *edges, int nseg, int64_t nrows, int c_in,
                      int c_out, hipStream_t st) {
#define SDP_BANDPASS_CASE(ND)                                                              \
    case ND:                                                                               \
        launch_polyfit<NC, ND>(gain, out, q, e, seg, edges, nseg, nrows, c_in, c_out, st); \
        break;
    switch (nd) {
        SDP_BANDPASS_CASE(1)
        SDP_BANDPASS_CASE(2)
        SDP_BANDPASS_CASE(3)
        SDP_BANDPASS_CASE(4)
        SDP_BANDPASS_CASE(5)
        SDP_BANDPASS_CASE(6)
        SDP_BANDPASS_CASE(7)
        SDP_BANDPASS_CASE(8)
        default:
            throw Error(SDP_HIP_ERR_INVALID_ARG, "polynomial degree out of range");
    }
#undef SDP_BANDPASS_CASE
}

void check_table(const void *gain, const void *out, int64_t nrows, int c_in, int c_out, int nrec) {
    SDP_REQUIRE(gain && out, "null pointer argument");
    SDP_REQUIRE(nrec == 1 || nrec == 2, "the gains must be 1 x 1 or 2 x 2 per channel");
    SDP_REQUIRE(nrows >= 1 && nrows < ((int64_t)1 << 31), "1 <= rows < 2^31");
    SDP_REQUIRE(c_in >= 1 && c_out >= 1 && c_in <= (1 << 24) && c_out <= (1 << 24),
                "1 <= input and output channels <= 2^24");
    SDP_REQUIRE(reinterpret_cast<uintptr_t>(gain) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(out) % 16 == 0,
                "gain and out must be aligned to 16 bytes");
}

}  // namespace bandpass
}  // namespace sdp

extern "C" {

int sdp_hip_resample_polyfit(int64_t nrows, int c_in, int c_out, int nrec, int degree, int nseg,
                             const void *gain, void *out, const double *q, const double *e,
                             const int32_t *seg, const int32_t *edges, void *stream, char *errbuf,
                             size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::bandpass;
    return guarded(errbuf, errbuf_len, [&] {
        check_table(gain, out, nrows, c_in, c_out, nrec);
        SDP_REQUIRE(q && e && seg && edges, "null pointer argument");
        SDP_REQUIRE(degree >= 0 && degree <= kMaxDegree,
                    "the device fit takes degrees 0 to " + std::to_string(kMaxDegree));
        SDP_REQUIRE(nseg >= 1 && nseg <= kMaxSegments,
                    "the device fit takes 1 to " + std::to_string(kMaxSegments) + " segments");
        SDP_REQUIRE(c_in >= 2, "resampling needs at least 2 input channels");
        const double *g = static_cast<const double *>(gain);
        double *o = static_cast<double *>(out);
        if (nrec == 2)
            dispatch_polyfit<8>(degree + 1, g, o, q, e, seg, edges, nseg, nrows, c_in, c_out,
                                as_stream(stream));
        else
            dispatch_polyfit<2>(degree + 1, g, o, q, e, seg, edges, nseg, nrows, c_in, c_out,
                                as_stream(stream));
    });
}

int sdp_hip_resample_interp(int64_t nrows, int c_in, int c_out, int nrec, const void *gain,
                            void *out, const double *x_in, const double *x_out,
                            const int32_t *interval, void *stream, char *errbuf,
                            size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::bandpass;
    return guarded(errbuf, errbuf_len, [&] {
        check_table(gain, out, nrows, c_in, c_out, nrec);
        SDP_REQUIRE(x_in && x_out && interval, "null pointer argument");
        const double *g = static_cast<const double *>(gain);
        double *o = static_cast<double *>(out);
        const int64_t total = nrows * c_out;
        const unsigned grid = (unsigned)std::min<int64_t>((total + kThreads - 1) / kThreads,
                                                          kInterpBlocks);
        if (nrec == 2)
            hipLaunchKernelGGL((k_interp<8>), dim3(grid), dim3(kThreads), 0, as_stream(stream), g, o,
                               x_in, x_out, interval, nrows, c_in, c_out);
        else
            hipLaunchKernelGGL((k_interp<2>), dim3(grid), dim3(kThreads), 0, as_stream(stream), g, o,
                               x_in, x_out, interval, nrows, c_in, c_out);
        SDP_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
