// The glue between imaging calls for gfx950 (reference src/
// ska_sdp_func_python/imaging/imaging_helpers.py): two streaming kernels behind
//   sdp_hip_sum_planes  out[p][i] = sum_n w[n][p] * in[n][p][i]  (/ sumwt[p]),
//                       or the plain sum out[p][i] = in[0][p][i] + in[1][p][i] + ...
//   sdp_hip_peak_abs    max over pol, y, x of |mean over channels| or of
//                       |the middle channel| of a cube that may be a strided view
// which serve sum_invert_results, sum_predict_results and threshold_list.
//
// sum_planes: every output element of the weighted mode starts from +0.0 and
// adds its terms in ascending n, product and sum each rounded once in fp64 (fp
// contraction is off), float32 inputs converted first, then is divided by
// sumwt[p] (a true division) or zeroed where sumwt[p] <= 0, and is rounded once
// more where the output is float32.  The plain mode adds in the element type.
// The N inputs are streamed past the accumulators of one group, so N costs no
// registers; every input is read once and the output written once, in one
// launch for all planes.  No LDS, nothing atomic.
//
// peak_abs: a thread owns a group of one row, sums it over the channels in
// fp64 and keeps the largest magnitude; the block's maximum goes to the result
// with one 64-bit integer atomicMax on the bit pattern of the non-negative
// fp64 value, which orders as the value does.  Max is order-independent, so
// the result is the same on every run.  NaN never wins a comparison: a thread
// that meets one stores 1 to a flag.
//
// As in taylor.hip a thread owns a group of 16 / sizeof(T) consecutive pixels;
// a plane or row whose first element is 16-byte aligned is accessed with one
// 16-byte access per lane, any other, and the group that holds the last pixels
// of a plane or row whose size is no multiple of the group, element by element.
#include "sdp_common.h"

#include <array>

#pragma clang fp contract(off)

namespace sdp {
namespace imgsum {

constexpr int kMaxCubes = SDP_HIP_SUM_PLANES_MAX;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1 << 13;  // groups beyond that are taken in a grid-stride loop
constexpr int64_t kMaxPix = (int64_t)1 << 40;

template <typename T>
struct Group;
template <>
struct Group<double> {
    static constexpr int V = 2;
    using vec = double2;
};
template <>
struct Group<float> {
    static constexpr int V = 4;
    using vec = float4;
};

__device__ __forceinline__ bool aligned16(const void *p) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// elements i0 .. i0 + V - 1 of the run p[0 .. n - 1]; elements past n read as 0
template <typename T>
__device__ __forceinline__ void load_group(const T *p, int64_t i0, int64_t n,
                                           T (&x)[Group<T>::V]) {
    constexpr int V = Group<T>::V;
    if (i0 + V <= n && aligned16(p)) {
        const typename Group<T>::vec v = *reinterpret_cast<const typename Group<T>::vec *>(p + i0);
        x[0] = v.x;
        x[1] = v.y;
        if constexpr (V == 4) {
            x[2] = v.z;
            x[3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = i0 + j < n ? p[i0 + j] : (T)0;
    }
}

template <typename T>
__device__ __forceinline__ void store_group(T *p, int64_t i0, int64_t n,
                                            const T (&a)[Group<T>::V]) {
    constexpr int V = Group<T>::V;
    if (i0 + V <= n && aligned16(p)) {
        typename Group<T>::vec v;
        v.x = a[0];
        v.y = a[1];
        if constexpr (V == 4) {
            v.z = a[2];
            v.w = a[3];
        }
        *reinterpret_cast<typename Group<T>::vec *>(p + i0) = v;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (i0 + j < n) p[i0 + j] = a[j];
    }
}

// plane p of cube n is in[n] + p * npix; wt is [ncube][nplane], sumwt [nplane].
// blockIdx.y strides over the planes, blockIdx.x over the groups of a plane.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_sum_weighted(int ncube, int64_t nplane, int64_t npix,
                                                           const void *const *__restrict__ in,
                                                           T *out, const double *__restrict__ wt,
                                                           const double *__restrict__ sumwt,
                                                           int normalise) {
    constexpr int V = Group<T>::V;
    const int64_t ngroups = (npix + V - 1) / V;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t p = blockIdx.y; p < nplane; p += gridDim.y) {
        const int64_t off = p * npix;
        const double s = normalise ? sumwt[p] : 1.0;
        for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += step) {
            const int64_t i0 = g * V;
            double acc[V];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.0;
#pragma unroll 4
            for (int n = 0; n < ncube; ++n) {
                T x[V];
                load_group<T>(static_cast<const T *>(in[n]) + off, i0, npix, x);
                const double w = wt[(size_t)n * nplane + p];
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = acc[j] + w * (double)x[j];
            }
            T r[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                double a = acc[j];
                if (normalise) a = s > 0.0 ? a / s : 0.0;
                r[j] = (T)a;
            }
            store_group<T>(out + off, i0, npix, r);
        }
    }
}

// out may be in[0]: a thread reads its group of every input before it writes
template <typename T>
__global__ __launch_bounds__(kThreads) void k_sum_plain(int ncube, int64_t nplane, int64_t npix,
                                                        const void *const *__restrict__ in,
                                                        T *out) {
    constexpr int V = Group<T>::V;
    const int64_t ngroups = (npix + V - 1) / V;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t p = blockIdx.y; p < nplane; p += gridDim.y) {
        const int64_t off = p * npix;
        for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += step) {
            const int64_t i0 = g * V;
            T acc[V];
            load_group<T>(static_cast<const T *>(in[0]) + off, i0, npix, acc);
#pragma unroll 4
            for (int n = 1; n < ncube; ++n) {
                T x[V];
                load_group<T>(static_cast<const T *>(in[n]) + off, i0, npix, x);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = acc[j] + x[j];
            }
            store_group<T>(out + off, i0, npix, acc);
        }
    }
}

template <typename T>
void run_sum(int ncube, int64_t nplane, int64_t npix, const void *const *in, void *out,
             const double *wt, const double *sumwt, int normalise, hipStream_t st) {
    constexpr int V = Group<T>::V;
    const int64_t ngroups = (npix + V - 1) / V;
    const unsigned gx = (unsigned)std::min<int64_t>((ngroups + kThreads - 1) / kThreads, kMaxBlocks);
    const unsigned gy = (unsigned)std::min<int64_t>(nplane, std::max<int64_t>(1, kMaxBlocks / gx));
    const dim3 grid(gx, gy);
    if (wt)
        k_sum_weighted<T><<<grid, kThreads, 0, st>>>(ncube, nplane, npix, in, static_cast<T *>(out),
                                                      wt, sumwt, normalise);
    else
        k_sum_plain<T><<<grid, kThreads, 0, st>>>(ncube, nplane, npix, in, static_cast<T *>(out));
    SDP_HIP_CHECK(hipGetLastError());
}

// result[0]: the bits of the peak; flag[0], flag[1]: a NaN was read, a mean was NaN
struct PeakOut {
    unsigned long long peak;
    int flag[2];
};

// A row is the nx elements from cube + c * cs + pol * ps + y * rs.  Flattened
// (row, group) items are taken in a grid-stride loop; their number fits 31 bits.
template <typename T, bool MOMENT>
__global__ __launch_bounds__(kThreads) void k_peak_abs(int nchan, int ny, int nx, unsigned nrows,
                                                       const T *cube, int64_t cs, int64_t ps,
                                                       int64_t rs, PeakOut *res) {
    constexpr int V = Group<T>::V;
    const unsigned gpr = (unsigned)((nx + V - 1) / V);
    const unsigned nitems = nrows * gpr;
    const unsigned step = gridDim.x * kThreads;
    const int c0 = MOMENT ? 0 : nchan / 2;
    const int c1 = MOMENT ? nchan : c0 + 1;
    const double div = (double)nchan;
    double best = 0.0;
    bool bad_in = false, bad_mean = false;
    // nitems < 2^31 and step <= 2^21: `it` cannot wrap
    for (unsigned it = blockIdx.x * kThreads + threadIdx.x; it < nitems; it += step) {
        const unsigned row = it / gpr;
        const unsigned gi = it - row * gpr;
        const unsigned pol = row / (unsigned)ny;
        const unsigned y = row - pol * (unsigned)ny;
        const T *p = cube + (int64_t)pol * ps + (int64_t)y * rs;
        const int64_t i0 = (int64_t)gi * V;
        double acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.0;
#pragma unroll 4
        for (int c = c0; c < c1; ++c) {
            T x[V];
            load_group<T>(p + (int64_t)c * cs, i0, nx, x);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double d = (double)x[j];
                bad_in |= d != d;
                acc[j] = MOMENT ? acc[j] + d : d;
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            double a = acc[j];
            if (MOMENT) {
                a = a / div;
                bad_mean |= a != a;
            }
            a = fabs(a);
            best = a > best ? a : best;  // a NaN never wins
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double other = __shfl_xor(best, o);
        best = other > best ? other : best;
    }
    __shared__ double wave_best[kWaves];
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) best = wave_best[w] > best ? wave_best[w] : best;
        if (best > 0.0) atomicMax(&res->peak, (unsigned long long)__double_as_longlong(best));
    }
    if (bad_in) res->flag[0] = 1;
    if (bad_mean) res->flag[1] = 1;
}

template <typename T>
void run_peak(int mode, int nchan, int npol, int ny, int nx, const void *cube, int64_t cs,
              int64_t ps, int64_t rs, PeakOut *res, hipStream_t st) {
    constexpr int V = Group<T>::V;
    const int64_t gpr = (nx + V - 1) / V;
    const int64_t nrows = (int64_t)npol * ny;
    SDP_REQUIRE(nrows * gpr < ((int64_t)1 << 31),
                "peak_abs takes at most 2^31 groups of 16 bytes per channel");
    const unsigned grid = (unsigned)std::min<int64_t>((nrows * gpr + kThreads - 1) / kThreads, kMaxBlocks);
    const T *c = static_cast<const T *>(cube);
    if (mode == SDP_HIP_PEAK_MOMENT0)
        k_peak_abs<T, true><<<grid, kThreads, 0, st>>>(nchan, ny, nx, (unsigned)nrows, c, cs, ps, rs, res);
    else
        k_peak_abs<T, false><<<grid, kThreads, 0, st>>>(nchan, ny, nx, (unsigned)nrows, c, cs, ps, rs, res);
    SDP_HIP_CHECK(hipGetLastError());
}

// The pointer table of a sum_planes call: written to pinned host memory,
// copied to the device buffer of the same slot on the call's stream.  A slot
// is reused only after the event recorded behind its last call has completed,
// so calls may be in flight on several streams without a synchronisation here.
constexpr int kSlots = 4;

struct Slot {
    void *host = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
};

struct Slots {
    std::array<Slot, kSlots> slot;
    int next = 0;
};

std::mutex g_mu;
std::map<int, Slots> g_slots;
std::map<int, PeakOut *> g_peak_host;  // pinned, one per device: peak_abs waits for its result

}  // namespace imgsum
}  // namespace sdp

extern "C" {

int sdp_hip_sum_planes(int ncube, int64_t nplane, int64_t npix, const void *const *in_cubes,
                       int dtype, void *out, const double *weights, const double *sumwt,
                       int normalise, void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::imgsum;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(ncube >= 1 && ncube <= kMaxCubes,
                    "sum_planes takes 1 .. " + std::to_string(kMaxCubes) + " inputs");
        SDP_REQUIRE(nplane >= 1 && npix >= 1 && npix <= kMaxPix && nplane <= kMaxPix / npix,
                    "the planes must hold 1 .. 2^40 pixels in all");
        SDP_REQUIRE(dtype == SDP_HIP_F32 || dtype == SDP_HIP_F64,
                    "the planes must be float32 or float64");
        SDP_REQUIRE(in_cubes && out, "null pointer argument");
        SDP_REQUIRE(!weights || sumwt || !normalise, "normalising needs sumwt");
        const size_t esize = dtype == SDP_HIP_F64 ? 8 : 4;
        for (int n = 0; n < ncube; ++n)
            SDP_REQUIRE(in_cubes[n] && reinterpret_cast<uintptr_t>(in_cubes[n]) % esize == 0,
                        "an input pointer is null or not aligned to its element");
        SDP_REQUIRE(reinterpret_cast<uintptr_t>(out) % esize == 0,
                    "the output pointer is not aligned to its element");
        const size_t span = (size_t)nplane * (size_t)npix * esize;
        const uintptr_t o_lo = reinterpret_cast<uintptr_t>(out);
        for (int n = 0; n < ncube; ++n) {
            const uintptr_t i_lo = reinterpret_cast<uintptr_t>(in_cubes[n]);
            if (!weights && n == 0 && i_lo == o_lo) continue;  // the plain sum onto its first input
            SDP_REQUIRE(o_lo + span <= i_lo || i_lo + span <= o_lo, "the output overlaps an input");
        }

        const size_t bytes = (size_t)ncube * sizeof(void *);
        const hipStream_t st = as_stream(stream);
        int dev = 0;
        SDP_HIP_CHECK(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_mu);
        Slots &ss = g_slots[dev];
        const int idx = ss.next;
        ss.next = (ss.next + 1) % kSlots;
        Slot &s = ss.slot[idx];
        if (!s.done) SDP_HIP_CHECK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        SDP_HIP_CHECK(hipEventSynchronize(s.done));  // an event never recorded counts as complete
        if (s.bytes < bytes) {
            if (s.host) SDP_HIP_CHECK(hipHostFree(s.host));
            s.host = nullptr;
            s.bytes = 0;
            SDP_HIP_CHECK(hipHostMalloc(&s.host, bytes + bytes / 8, hipHostMallocDefault));
            s.bytes = bytes + bytes / 8;
        }
        std::memcpy(s.host, in_cubes, bytes);
        char *d = scratch<char>("sum_planes_table" + std::to_string(idx), bytes);
        SDP_HIP_CHECK(hipMemcpyAsync(d, s.host, bytes, hipMemcpyHostToDevice, st));
        const void *const *tab = reinterpret_cast<const void *const *>(d);
        if (dtype == SDP_HIP_F64)
            run_sum<double>(ncube, nplane, npix, tab, out, weights, sumwt, normalise, st);
        else
            run_sum<float>(ncube, nplane, npix, tab, out, weights, sumwt, normalise, st);
        SDP_HIP_CHECK(hipEventRecord(s.done, st));
    });
}

int sdp_hip_peak_abs(int mode, int nchan, int npol, int ny, int nx, const void *cube, int dtype,
                     int64_t chan_stride, int64_t pol_stride, int64_t row_stride, double *peak,
                     int *nan_seen, void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::imgsum;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(mode == SDP_HIP_PEAK_MOMENT0 || mode == SDP_HIP_PEAK_REFCHAN,
                    "peak_abs: unknown mode");
        SDP_REQUIRE(nchan >= 1 && npol >= 1 && ny >= 1 && nx >= 1, "peak_abs needs a non-empty cube");
        SDP_REQUIRE(dtype == SDP_HIP_F32 || dtype == SDP_HIP_F64,
                    "the cube must be float32 or float64");
        SDP_REQUIRE(cube && peak && nan_seen, "null pointer argument");
        SDP_REQUIRE(chan_stride >= 0 && pol_stride >= 0 && row_stride >= 0,
                    "the strides must not be negative");
        const size_t esize = dtype == SDP_HIP_F64 ? 8 : 4;
        SDP_REQUIRE(reinterpret_cast<uintptr_t>(cube) % esize == 0,
                    "the cube pointer is not aligned to its element");

        const hipStream_t st = as_stream(stream);
        int dev = 0;
        SDP_HIP_CHECK(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_mu);
        PeakOut *&h = g_peak_host[dev];
        if (!h) SDP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&h), sizeof(PeakOut), hipHostMallocDefault));
        PeakOut *d = scratch<PeakOut>("peak_abs_result", 1);
        SDP_HIP_CHECK(hipMemsetAsync(d, 0, sizeof(PeakOut), st));
        if (dtype == SDP_HIP_F64)
            run_peak<double>(mode, nchan, npol, ny, nx, cube, chan_stride, pol_stride, row_stride, d, st);
        else
            run_peak<float>(mode, nchan, npol, ny, nx, cube, chan_stride, pol_stride, row_stride, d, st);
        SDP_HIP_CHECK(hipMemcpyAsync(h, d, sizeof(PeakOut), hipMemcpyDeviceToHost, st));
        SDP_HIP_CHECK(hipStreamSynchronize(st));
        double v;
        std::memcpy(&v, &h->peak, sizeof v);
        *nan_seen = (h->flag[0] ? SDP_HIP_PEAK_NAN_INPUT : 0) | (h->flag[1] ? SDP_HIP_PEAK_NAN_MEAN : 0);
        *peak = v;
    });
}

}  // extern "C"
