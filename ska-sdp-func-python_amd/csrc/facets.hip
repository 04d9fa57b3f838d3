// Gather of image facets for gfx950 (reference src/ska_sdp_func_python/image/
// gather_scatter.py:53-166 with the raster of image/iterators.py:123-190): one
// streaming kernel behind
//   sdp_hip_gather_facets   out[p][y][x] = sum_f wt_f v_f / sum_f wt_f
// over the facets f that cover pixel (y, x), in ascending fy, then ascending
// fx, the order in which the reference adds them into its output image.
//
// Per output element, in the image's type T (fp contraction is off):
//   acc = +0, sum = +0
//   wt  = (T)(taper_y[j] * taper_x[i])    product in fp64, then cast: how numpy
//                                          fills the reference's "flat" images
//   acc = acc + wt * v,  sum = sum + wt    (no tapers: wt = 1, acc = acc + v)
//   out = normalise ? (sum > 0 ? acc / sum : 0) : acc
// A pixel that no facet covers gets +0.  Every facet pixel is read once and
// every output pixel written once; no full-size temporaries, no masked passes.
//
// The grid is x tile by band of kRows rows by plane, so the fy range is uniform
// in a block and its x tile fixed: a thread owns kBytes / sizeof(T) consecutive
// x of each row of the band, and what depends on x alone (the fx range, the x
// taper of its first two facets) is found once per block, while the block
// strides over bands and planes.  The facets that cover a band or a run of x
// follow by division from the origin, the step and the facet size (more than
// two per axis once 4 * overlap > facet size).  A facet row starts at any x of
// any allocation, so it is read with loads that assume the alignment of one
// element only; the output row is written 16 bytes at a time where it is
// aligned so.  The facet pointers and strides and the tapers are read from
// tables in device memory.  No LDS, nothing atomic.
#include "sdp_common.h"

#include <array>

#pragma clang fp contract(off)

namespace sdp {
namespace facets {

constexpr int kMaxFacets = SDP_HIP_GATHER_FACETS_MAX;
constexpr int kThreads = 256;
// 32 bytes of 2 rows per thread: of 16 or 32 bytes by 1, 2 or 4 rows the
// fastest on the 8192^2 bench shape, if by a few per cent only
constexpr int kBytes = 32;  // of one output row per thread
constexpr int kRows = 2;    // output rows per thread
constexpr int kMaxBlocks = 1 << 14;  // of a launch, about: the grid strides over the rest
constexpr int kMaxSide = 1 << 30;
constexpr int64_t kMaxPix = (int64_t)1 << 40;

struct Geometry {
    int facets, nplanes, ny, nx, dy, dx, y0, x0, sy, sx, normalise;
};

struct Tables {
    const void *const *ptr;    // [facets^2] first element of each facet, or NULL (weights only)
    const int64_t *pstride;    // [facets^2] elements between planes
    const int64_t *rstride;    // [facets^2] elements between rows
    const double *taper_y;     // [dy] or NULL
    const double *taper_x;     // [dx] or NULL
};

// A pointer read from a table in memory is generic to the compiler; this marks
// it as one into global memory (device pass only)
#if defined(__HIP_DEVICE_COMPILE__)
#define SDP_GLOBAL __attribute__((address_space(1)))
#else
#define SDP_GLOBAL
#endif

// V elements of T that are aligned as one element only
template <typename T, int V>
struct __attribute__((packed, aligned(sizeof(T)))) Run {
    T v[V];
};

__device__ __forceinline__ bool aligned16(const void *p) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// the facets f in 0 .. F - 1 with f * s <= t < f * s + d, for t_lo <= t <= t_hi
__device__ __forceinline__ void cover(int t_lo, int t_hi, int s, int d, int F, int &lo, int &hi) {
    lo = t_lo >= d ? (t_lo - d) / s + 1 : 0;
    hi = t_hi < 0 ? -1 : min(F - 1, t_hi / s);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_gather_facets(Geometry g, Tables t,
                                                            T *__restrict__ out,
                                                            T *__restrict__ sumwt) {
    constexpr int V = kBytes / (int)sizeof(T);
    constexpr int R = kRows;
    constexpr int kTile = kThreads * V;
    using GlobalPtr = const SDP_GLOBAL T *;
    using GlobalRun = const SDP_GLOBAL Run<T, V> *;
    const int nty = (g.ny + R - 1) / R;
    const bool tapered = t.taper_y != nullptr;
    const bool read = t.ptr != nullptr;
    // the block's x tile is fixed, so all that depends on x alone is found once
    const int xg = (int)blockIdx.x * kTile + (int)threadIdx.x * V;
    if (xg >= g.nx) return;
    const int nvalid = min(V, g.nx - xg);
    int fx_lo, fx_hi;
    cover(xg - g.x0, xg + nvalid - 1 - g.x0, g.sx, g.dx, g.facets, fx_lo, fx_hi);
    // the x taper of the first two facets of the range stays in registers
    double tx_a[V], tx_b[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int ia = xg + k - g.x0 - fx_lo * g.sx, ib = ia - g.sx;
        tx_a[k] = tapered && fx_lo <= fx_hi && k < nvalid && ia >= 0 && ia < g.dx ? t.taper_x[ia] : 1.0;
        tx_b[k] = tapered && fx_lo < fx_hi && k < nvalid && ib >= 0 && ib < g.dx ? t.taper_x[ib] : 1.0;
    }
    for (int64_t plane = blockIdx.z; plane < g.nplanes; plane += gridDim.z)
    for (int band = blockIdx.y; band < nty; band += gridDim.y) {
        const int yb = band * R;
        const int nrows = min(R, g.ny - yb);

        T acc[R][V], sum[R][V];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < V; ++k) acc[r][k] = sum[r][k] = (T)0;

        int fy_lo, fy_hi;
        cover(yb - g.y0, yb + nrows - 1 - g.y0, g.sy, g.dy, g.facets, fy_lo, fy_hi);
        for (int fy = fy_lo; fy <= fy_hi; ++fy) {
            const int j0 = yb - g.y0 - fy * g.sy;  // facet row of the band's first row
            bool row_in[R];
            double ty[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                row_in[r] = r < nrows && j0 + r >= 0 && j0 + r < g.dy;
                ty[r] = row_in[r] && tapered ? t.taper_y[j0 + r] : 1.0;
            }
            for (int fx = fx_lo; fx <= fx_hi; ++fx) {
                const int i0 = xg - g.x0 - fx * g.sx;  // facet column of the first element
                const int f = fy * g.facets + fx;
                GlobalPtr base = nullptr;
                int64_t rstride = 0;
                if (read) {
                    rstride = t.rstride[f];
                    base = (GlobalPtr)(static_cast<const T *>(t.ptr[f]) + plane * t.pstride[f]);
                }
                const bool whole = i0 >= 0 && i0 + V <= g.dx && nvalid == V;
                T v[R][V];
                double tx[V];
                bool in[V];
#pragma unroll
                for (int k = 0; k < V; ++k) in[k] = whole || (k < nvalid && i0 + k >= 0 && i0 + k < g.dx);
                if (read) {
                    if (whole) {
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            if (!row_in[r]) continue;
                            const GlobalRun run = (GlobalRun)(base + (j0 + r) * rstride + i0);
#pragma unroll
                            for (int k = 0; k < V; ++k) v[r][k] = run->v[k];
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int k = 0; k < V; ++k)
                                v[r][k] = row_in[r] && in[k] ? base[(j0 + r) * rstride + i0 + k] : (T)0;
                    }
                }
                if (tapered) {
#pragma unroll
                    for (int k = 0; k < V; ++k) tx[k] = fx == fx_lo ? tx_a[k] : tx_b[k];
                    if (fx > fx_lo + 1) {
#pragma unroll
                        for (int k = 0; k < V; ++k) tx[k] = in[k] ? t.taper_x[i0 + k] : 1.0;
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (!row_in[r]) continue;
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        if (!in[k]) continue;
                        if (tapered) {
                            const T wt = (T)(ty[r] * tx[k]);
                            if (read) acc[r][k] = acc[r][k] + wt * v[r][k];
                            sum[r][k] = sum[r][k] + wt;
                        } else {
                            if (read) acc[r][k] = acc[r][k] + v[r][k];
                            sum[r][k] = sum[r][k] + (T)1;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (g.normalise)
                    acc[r][k] = sum[r][k] > (T)0 ? acc[r][k] / sum[r][k] : (T)0;
                else
                    sum[r][k] = (T)1;  // nothing to divide by: the reference's flat of ones
            }

        const int64_t o = (plane * g.ny + yb) * g.nx + xg;
        T *const dst[2] = {out, sumwt};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            if (!dst[w]) continue;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= nrows) continue;
                T *p = dst[w] + o + (int64_t)r * g.nx;
                const T *src = w ? sum[r] : acc[r];
                if (nvalid == V && aligned16(p)) {
                    constexpr int Q = 16 / (int)sizeof(T);
                    struct alignas(16) Quad {
                        T v[Q];
                    };
#pragma unroll
                    for (int k = 0; k < V; k += Q) {
                        Quad q;
#pragma unroll
                        for (int m = 0; m < Q; ++m) q.v[m] = src[k + m];
                        *reinterpret_cast<Quad *>(p + k) = q;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k)
                        if (k < nvalid) p[k] = src[k];
                }
            }
        }
    }
}

template <typename T>
void run(const Geometry &g, const Tables &t, void *out, void *sumwt, hipStream_t st) {
    constexpr int kTile = kThreads * (kBytes / (int)sizeof(T));
    // x tile, band of rows, plane; bands and planes beyond the grid are taken in strides
    const int ntx = (g.nx + kTile - 1) / kTile;
    const int nty = (g.ny + kRows - 1) / kRows;
    const int gz = std::min(g.nplanes, std::max(1, kMaxBlocks / ntx));
    const int gy = std::min(nty, std::max(1, kMaxBlocks / (ntx * gz)));
    k_gather_facets<T><<<dim3(ntx, gy, gz), kThreads, 0, st>>>(g, t, static_cast<T *>(out),
                                                              static_cast<T *>(sumwt));
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

}  // namespace facets
}  // namespace sdp

extern "C" {

int sdp_hip_gather_facets(int dtype, int facets, int nplanes, int ny, int nx, int dy, int dx,
                          int y0, int x0, int sy, int sx, const void *const *facet_ptrs,
                          const int64_t *plane_strides, const int64_t *row_strides,
                          const double *taper_y, const double *taper_x, int normalise,
                          void *out, void *sumwt, void *stream, char *errbuf,
                          size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::facets;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(dtype == SDP_HIP_F32 || dtype == SDP_HIP_F64,
                    "the facets must be float32 or float64");
        SDP_REQUIRE(facets >= 1 && facets <= kMaxFacets,
                    "gather_facets takes 1 .. " + std::to_string(kMaxFacets) +
                        " facets per axis");
        SDP_REQUIRE(nplanes >= 1 && ny >= 1 && nx >= 1 && ny <= kMaxSide && nx <= kMaxSide &&
                        (int64_t)nplanes * ny * nx <= kMaxPix,
                    "the image must have 1 .. 2^30 pixels per side and at most 2^40 in all");
        SDP_REQUIRE(dy >= 1 && dx >= 1 && dy <= ny && dx <= nx,
                    "the facet size must be 1 .. the image size on each axis");
        SDP_REQUIRE(sy >= 1 && sx >= 1, "the steps between facets must be at least 1");
        SDP_REQUIRE(y0 >= 0 && (int64_t)y0 + (int64_t)(facets - 1) * sy + dy <= ny,
                    "the facets leave the image in y");
        SDP_REQUIRE(x0 >= 0 && (int64_t)x0 + (int64_t)(facets - 1) * sx + dx <= nx,
                    "the facets leave the image in x");
        SDP_REQUIRE(out || sumwt, "gather_facets needs an output");
        SDP_REQUIRE((taper_y == nullptr) == (taper_x == nullptr),
                    "taper_y and taper_x come together or not at all");
        SDP_REQUIRE(!out || (facet_ptrs && plane_strides && row_strides),
                    "null pointer argument");
        const size_t esize = dtype == SDP_HIP_F64 ? 8 : 4;
        const size_t nf = (size_t)facets * facets;
        const bool read = out != nullptr;
        if (read)
            for (size_t f = 0; f < nf; ++f) {
                SDP_REQUIRE(facet_ptrs[f] && reinterpret_cast<uintptr_t>(facet_ptrs[f]) % esize == 0,
                            "a facet pointer is null or not aligned to its element");
                SDP_REQUIRE(plane_strides[f] >= 0 && row_strides[f] >= 0,
                            "a facet stride is negative");
            }
        for (void *p : {out, sumwt})
            SDP_REQUIRE(reinterpret_cast<uintptr_t>(p) % esize == 0,
                        "an output pointer is not aligned to its element");

        const size_t off_ps = round16(nf * sizeof(void *));
        const size_t off_rs = off_ps + round16(nf * sizeof(int64_t));
        const size_t off_ty = off_rs + round16(nf * sizeof(int64_t));
        const size_t off_tx = off_ty + round16((size_t)dy * sizeof(double));
        const size_t bytes = off_tx + round16((size_t)dx * sizeof(double));

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
        std::memset(h, 0, bytes);
        if (read) {
            std::memcpy(h, facet_ptrs, nf * sizeof(void *));
            std::memcpy(h + off_ps, plane_strides, nf * sizeof(int64_t));
            std::memcpy(h + off_rs, row_strides, nf * sizeof(int64_t));
        }
        if (taper_y) {
            std::memcpy(h + off_ty, taper_y, (size_t)dy * sizeof(double));
            std::memcpy(h + off_tx, taper_x, (size_t)dx * sizeof(double));
        }

        char *d = scratch<char>("gather_facets_tables" + std::to_string(idx), bytes);
        SDP_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
        Tables t;
        t.ptr = read ? reinterpret_cast<const void *const *>(d) : nullptr;
        t.pstride = reinterpret_cast<const int64_t *>(d + off_ps);
        t.rstride = reinterpret_cast<const int64_t *>(d + off_rs);
        t.taper_y = taper_y ? reinterpret_cast<const double *>(d + off_ty) : nullptr;
        t.taper_x = taper_y ? reinterpret_cast<const double *>(d + off_tx) : nullptr;
        const Geometry g{facets, nplanes, ny, nx, dy, dx, y0, x0, sy, sx, normalise ? 1 : 0};
        if (dtype == SDP_HIP_F64)
            run<double>(g, t, out, sumwt, st);
        else
            run<float>(g, t, out, sumwt, st);
        SDP_HIP_CHECK(hipEventRecord(s.done, st));
    });
}

}  // extern "C"
