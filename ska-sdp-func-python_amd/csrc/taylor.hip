// Frequency Taylor terms of image stacks for gfx950 (reference src/
// ska_sdp_func_python/image/taylor_terms.py): one streaming kernel pair behind
//   sdp_hip_mix_planes    out[k][i] = sum_c w[k][c] * in[c][i]
// which serves the moments of a cube or an image list (few outputs, many
// inputs), the channels rebuilt from Taylor terms (many outputs, few inputs)
// and the decoupled Taylor terms (w = pinv of the coupling matrix).
//
// Every output element starts from +0.0 and adds its terms in ascending c,
// product and sum each rounded once in fp64 (fp contraction is off), float32
// inputs converted first: numpy's `out[k] += in[c] * w`, bit for bit.
//
// A thread owns a group of 16 / sizeof(T) consecutive pixels, so a
// plane whose pointer is 16-byte aligned is read or written with one 16-byte
// access per lane; any other plane, and the group that holds the last pixels
// of a plane whose size is no multiple of the group, is accessed element by
// element.  "Reduce" holds up to kRegs accumulators per pixel in registers and
// streams the input planes past them; "expand" holds up to kRegs input planes
// and streams the outputs.  With min(nin, nout) <= kRegs every plane is read
// once and written once.  Beyond that the outputs are split into reduce passes
// of kRegs, each of which reads all inputs again: nin ceil(nout / kRegs) + nout
// planes moved.  (Expand passes over kRegs inputs at a time, continuing from
// the stored partial sums, would give the same bits but read and write every
// output in each pass, nin + (2 ceil(nin / kRegs) - 1) nout planes, which is
// never fewer once nin > kRegs.)
// The plane pointers and the weights are read from a table in device memory
// with wave-uniform indices.  No LDS, nothing atomic.
#include "sdp_common.h"

#include <array>
#include <type_traits>

#pragma clang fp contract(off)

namespace sdp {
namespace taylor {

constexpr int kRegs = SDP_HIP_MIX_PLANES_REGS;
constexpr int kMaxPlanes = SDP_HIP_MIX_PLANES_MAX;
constexpr int kThreads = 256;
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

// pixels i0 .. i0 + V - 1 of plane p as fp64; pixels past npix read as 0
template <typename T>
__device__ __forceinline__ void load_group(const T *p, int64_t i0, int64_t npix,
                                           double (&x)[Group<T>::V], bool &bad) {
    constexpr int V = Group<T>::V;
    if (i0 + V <= npix && aligned16(p)) {
        const typename Group<T>::vec v = *reinterpret_cast<const typename Group<T>::vec *>(p + i0);
        if constexpr (V == 2) {
            x[0] = v.x;
            x[1] = v.y;
        } else {
            x[0] = (double)v.x;
            x[1] = (double)v.y;
            x[2] = (double)v.z;
            x[3] = (double)v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = i0 + j < npix ? (double)p[i0 + j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) bad |= x[j] != x[j];
}

// V fp64 pixels from i0 on: 16-byte stores into an aligned plane
template <int V>
__device__ __forceinline__ void store_group(double *p, int64_t i0, int64_t npix,
                                            const double (&a)[V], bool &bad) {
    if (i0 + V <= npix && aligned16(p)) {
#pragma unroll
        for (int j = 0; j < V; j += 2) {
            *reinterpret_cast<double2 *>(p + i0 + j) = make_double2(a[j], a[j + 1]);
            bad |= a[j] != a[j] || a[j + 1] != a[j + 1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (i0 + j < npix) {
                p[i0 + j] = a[j];
                bad |= a[j] != a[j];
            }
    }
}

// outputs k0 .. k0 + K - 1 from all nin inputs; wt is [nin][nout]
template <typename T, int K>
__global__ __launch_bounds__(kThreads) void k_mix_reduce(int nin, int nout, int k0, int64_t npix,
                                                         const void *const *__restrict__ in,
                                                         double *const *__restrict__ out,
                                                         const double *__restrict__ wt,
                                                         int *nan_flag) {
    constexpr int V = Group<T>::V;
    const int64_t ngroups = (npix + V - 1) / V;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    bool bad_in = false, bad_out = false;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += step) {
        const int64_t i0 = g * V;
        double acc[K][V];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) acc[k][j] = 0.0;
#pragma unroll 4
        for (int c = 0; c < nin; ++c) {
            double x[V];
            load_group<T>(static_cast<const T *>(in[c]), i0, npix, x, bad_in);
            const double *w = wt + (size_t)c * nout + k0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double wk = w[k];
#pragma unroll
                for (int j = 0; j < V; ++j) acc[k][j] = acc[k][j] + wk * x[j];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) store_group<V>(out[k0 + k], i0, npix, acc[k], bad_out);
    }
    if (nan_flag) {
        if (bad_in) nan_flag[0] = 1;
        if (bad_out) nan_flag[1] = 1;
    }
}

// all nout outputs from the C inputs; w is [nout][C]
template <typename T, int C>
__global__ __launch_bounds__(kThreads) void k_mix_expand(int nout, int64_t npix,
                                                         const void *const *__restrict__ in,
                                                         double *const *__restrict__ out,
                                                         const double *__restrict__ w,
                                                         int *nan_flag) {
    constexpr int V = Group<T>::V;
    const int64_t ngroups = (npix + V - 1) / V;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    bool bad_in = false, bad_out = false;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += step) {
        const int64_t i0 = g * V;
        double x[C][V];
#pragma unroll
        for (int c = 0; c < C; ++c)
            load_group<T>(static_cast<const T *>(in[c]), i0, npix, x[c], bad_in);
#pragma unroll 2
        for (int k = 0; k < nout; ++k) {
            double acc[V];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.0;
            const double *wk = w + (size_t)k * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double wc = wk[c];
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = acc[j] + wc * x[c][j];
            }
            store_group<V>(out[k], i0, npix, acc, bad_out);
        }
    }
    if (nan_flag) {
        if (bad_in) nan_flag[0] = 1;
        if (bad_out) nan_flag[1] = 1;
    }
}

struct Tables {
    const void *const *in;
    double *const *out;
    const double *w;   // [nout][nin]
    const double *wt;  // [nin][nout]
    int *nan_flag;  // [2]: a NaN was read from an input, written to an output; or NULL
};

template <typename T, int K>
void launch_reduce(unsigned grid, hipStream_t st, int nin, int nout, int k0, int64_t npix,
                   const Tables &t) {
    k_mix_reduce<T, K><<<grid, kThreads, 0, st>>>(nin, nout, k0, npix, t.in, t.out, t.wt, t.nan_flag);
}

template <typename T, int C>
void launch_expand(unsigned grid, hipStream_t st, int nout, int64_t npix, const Tables &t) {
    k_mix_expand<T, C><<<grid, kThreads, 0, st>>>(nout, npix, t.in, t.out, t.w, t.nan_flag);
}

// call fn(integral_constant<int, n>) for the run-time n in 1 .. kRegs
template <int N = kRegs, class F>
void with_count(int n, F &&fn) {
    if constexpr (N >= 1) {
        if (n == N)
            fn(std::integral_constant<int, N>{});
        else
            with_count<N - 1>(n, fn);
    }
}

template <typename T>
void run(int nin, int nout, int64_t npix, const Tables &t, hipStream_t st) {
    constexpr int V = Group<T>::V;
    const int64_t ngroups = (npix + V - 1) / V;
    const unsigned grid = (unsigned)std::min<int64_t>((ngroups + kThreads - 1) / kThreads, kMaxBlocks);
    if (nout > kRegs && nin <= kRegs) {
        with_count(nin, [&](auto c) { launch_expand<T, decltype(c)::value>(grid, st, nout, npix, t); });
    } else {
        for (int k0 = 0; k0 < nout; k0 += kRegs)
            with_count(std::min(kRegs, nout - k0), [&](auto k) {
                launch_reduce<T, decltype(k)::value>(grid, st, nin, nout, k0, npix, t);
            });
    }
    SDP_HIP_CHECK(hipGetLastError());
}

// The tables of a call: written to pinned host memory, copied to the device
// buffer of the same slot on the call's stream.  A slot is reused only after
// the event recorded behind its last call has completed, so calls may be in
// flight on several streams without a synchronisation here.
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

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace taylor
}  // namespace sdp

extern "C" {

int sdp_hip_mix_planes(int nin, int nout, int64_t npix, const void *const *in_planes,
                       int in_dtype, double *const *out_planes, const double *weights,
                       int *nan_seen, void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::taylor;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(nin >= 1 && nout >= 1, "mix_planes needs at least one input and one output plane");
        SDP_REQUIRE(nin <= kMaxPlanes && nout <= kMaxPlanes,
                    "mix_planes takes at most " + std::to_string(kMaxPlanes) +
                        " input and as many output planes");
        SDP_REQUIRE(npix >= 1 && npix <= kMaxPix, "the plane size must be 1 .. 2^40 pixels");
        SDP_REQUIRE(in_dtype == SDP_HIP_F32 || in_dtype == SDP_HIP_F64,
                    "the input planes must be float32 or float64");
        SDP_REQUIRE(in_planes && out_planes && weights, "null pointer argument");
        const size_t esize = in_dtype == SDP_HIP_F64 ? 8 : 4;
        for (int c = 0; c < nin; ++c)
            SDP_REQUIRE(in_planes[c] && reinterpret_cast<uintptr_t>(in_planes[c]) % esize == 0,
                        "an input plane pointer is null or not aligned to its element");
        for (int k = 0; k < nout; ++k)
            SDP_REQUIRE(out_planes[k] && reinterpret_cast<uintptr_t>(out_planes[k]) % 8 == 0,
                        "an output plane pointer is null or not aligned to its element");

        const size_t nw = (size_t)nin * nout;
        const size_t off_out = round16((size_t)nin * sizeof(void *));
        const size_t off_w = off_out + round16((size_t)nout * sizeof(void *));
        const size_t off_wt = off_w + nw * sizeof(double);
        const size_t off_flag = off_wt + nw * sizeof(double);
        const size_t bytes = off_flag + 16;

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
        char *h = static_cast<char *>(s.host);
        std::memcpy(h, in_planes, (size_t)nin * sizeof(void *));
        std::memcpy(h + off_out, out_planes, (size_t)nout * sizeof(void *));
        std::memcpy(h + off_w, weights, nw * sizeof(double));
        double *wt = reinterpret_cast<double *>(h + off_wt);
        for (int k = 0; k < nout; ++k)
            for (int c = 0; c < nin; ++c) wt[(size_t)c * nout + k] = weights[(size_t)k * nin + c];
        std::memset(h + off_flag, 0, 16);

        char *d = scratch<char>("mix_planes_tables" + std::to_string(idx), bytes);
        SDP_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
        Tables t;
        t.in = reinterpret_cast<const void *const *>(d);
        t.out = reinterpret_cast<double *const *>(d + off_out);
        t.w = reinterpret_cast<const double *>(d + off_w);
        t.wt = reinterpret_cast<const double *>(d + off_wt);
        t.nan_flag = nan_seen ? reinterpret_cast<int *>(d + off_flag) : nullptr;
        if (in_dtype == SDP_HIP_F64)
            run<double>(nin, nout, npix, t, st);
        else
            run<float>(nin, nout, npix, t, st);
        if (nan_seen) {
            SDP_HIP_CHECK(hipMemcpyAsync(h + off_flag, d + off_flag, 2 * sizeof(int),
                                         hipMemcpyDeviceToHost, st));
            SDP_HIP_CHECK(hipStreamSynchronize(st));
            const int *f = reinterpret_cast<const int *>(h + off_flag);
            *nan_seen = (f[0] ? SDP_HIP_MIX_NAN_INPUT : 0) | (f[1] ? SDP_HIP_MIX_NAN_OUTPUT : 0);
        } else {
            SDP_HIP_CHECK(hipEventRecord(s.done, st));
        }
    });
}

}  // extern "C"
