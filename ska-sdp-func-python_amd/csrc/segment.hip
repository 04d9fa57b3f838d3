// Image segmentation for gfx950: the device half of find_skycomponents
// (reference src/ska_sdp_func_python/sky_component/operations.py:256-363, which
// reaches it through photutils' detect_sources and SourceCatalog):
//   sdp_hip_segment_label    channel mean of the planes, Gaussian smoothing,
//                            threshold, 8-connected labelling, segment sizes
//   sdp_hip_segment_roots    the roots of the segments that are large enough
//   sdp_hip_segment_relabel  the segment map 1..n, 0 = background
//   sdp_hip_segment_peaks    per (plane, segment) the maximum and its first pixel
//
// Labelling is a union-find over the pixels in which a parent is always a
// pixel of smaller flat index, so the root of a component is its first pixel
// in raster order whatever the schedule:
//   k_segment_tiles   a workgroup owns a kTile x kTile tile: it forms the mean
//                     plane with a halo in LDS, smooths, thresholds, joins the
//                     tile's pixels in an LDS union-find, and writes per pixel
//                     the flat index of its tile-local root (-1: background)
//                     and per tile-local root its pixel count;
//   k_segment_merge   one thread per pixel of a tile's first row or column
//                     joins it with its (up to three) neighbours in the tile
//                     before, diagonals and tile corners included, in global
//                     memory: atomicMin at device scope decides, relaxed
//                     device-scope loads only guide the walk;
//   k_segment_flatten every pixel takes its root (path compression) and every
//                     tile-local root adds its count to that root.
// A kernel ends before the next begins (stream order); no workgroup waits for
// another.  A walk to a root follows strictly decreasing indices and a join
// strictly decreases the sum of the two indices it holds: every loop is bounded
// by the data.  Counts and peaks use integer atomics only: all results are
// functions of the input alone.  fp contraction is off.
#include "sdp_common.h"

#pragma clang fp contract(off)

namespace sdp {
namespace segment {

constexpr int kTile = SDP_HIP_SEGMENT_TILE;
constexpr int kThreads = 256;
constexpr int kRows = kThreads / kTile;         // tile rows the threads cover at once
constexpr int kPerThread = kTile / kRows;       // pixels of a thread
constexpr int kMaxK = SDP_HIP_SEGMENT_KERNEL_MAX;
constexpr int kMaxW = kTile + kMaxK - 1;        // tile side with the halo
constexpr int kMaxBlocks = 1 << 16;             // more tiles are taken in a grid-stride loop

static_assert(kTile == 32 && kThreads % kTile == 0 && kTile % kRows == 0,
              "the kernels take lane & 31 as the tile column");

// ---- union-find with the smaller index as parent -----------------------------
struct LdsOps {  // a tile's labels in LDS
    static __device__ __forceinline__ int load(const int *p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ int min(int *p, int v) {
        return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
struct GlobalOps {  // the image's labels: other workgroups, other XCDs
    static __device__ __forceinline__ int load(const int *p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ int min(int *p, int v) {
        return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// the root of x: parents decrease strictly, a root is its own parent
template <class Ops>
__device__ __forceinline__ int find_root(const int *L, int x) {
    for (int p = Ops::load(L + x); p != x; p = Ops::load(L + x)) x = p;
    return x;
}

// Join the sets of a and b.  A value read by find_root may be out of date (it
// is then a former, larger ancestor); what atomicMin returns is not.  Where the
// larger root a has meanwhile been given a parent `old`, a's link is the
// smaller of old and b and the join goes on with (old, b), which restores
// whichever link was dropped.
template <class Ops>
__device__ __forceinline__ void join(int *L, int a, int b) {
    for (;;) {
        a = find_root<Ops>(L, a);
        b = find_root<Ops>(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = Ops::min(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// ---- mean, smoothing, threshold, tile-local labels --------------------------
struct TileArgs {
    const void *planes;
    int64_t plane_stride;
    int nchan, ny, nx, ksize;
    double threshold, tap_sum;
    int32_t *labels, *count, *nonfinite;
    int tiles_x;
    int64_t ntiles;
    double taps[kMaxK * kMaxK];
};

// numpy.sum over the channel axis, then one division, in the pixel type (:287)
template <typename T>
__device__ __forceinline__ double mean_of(const T *pix, int64_t stride, int nchan) {
    T acc = pix[0];
    for (int c = 1; c < nchan; ++c) acc = acc + pix[(size_t)c * stride];
    return (double)(acc / (T)nchan);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_segment_tiles(TileArgs a) {
    __shared__ double s_mean[kMaxW * kMaxW];
    __shared__ double s_taps[kMaxK * kMaxK];
    __shared__ int s_lab[kTile * kTile], s_cnt[kTile * kTile];
    const int K = a.ksize, h = K / 2, W = kTile + 2 * h;
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x / kTile;
    const T *planes = static_cast<const T *>(a.planes);
    for (int e = threadIdx.x; e < K * K; e += kThreads) s_taps[e] = a.taps[e];
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int x0 = (int)(tile % a.tiles_x) * kTile, y0 = (int)(tile / a.tiles_x) * kTile;
        bool bad = false;
        __syncthreads();  // the tile before is done with LDS
        for (int e = threadIdx.x; e < W * W; e += kThreads) {
            const int y = y0 - h + e / W, x = x0 - h + e % W;
            double m = 0.0;  // pixels off the image count as 0
            if (y >= 0 && y < a.ny && x >= 0 && x < a.nx) {
                m = mean_of<T>(planes + (size_t)y * a.nx + x, a.plane_stride, a.nchan);
                bad |= !isfinite(m);
            }
            s_mean[e] = m;
        }
        if (bad) atomicOr(a.nonfinite, 1);
        __syncthreads();
        bool fg[kPerThread];
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) {
            const int y = ly + r * kRows;
            double acc = 0.0;
            for (int dy = 0; dy < K; ++dy)
                for (int dx = 0; dx < K; ++dx)
                    acc = acc + s_mean[(y + dy) * W + lx + dx] * s_taps[dy * K + dx];
            const double smooth = acc / a.tap_sum;
            fg[r] = y0 + y < a.ny && x0 + lx < a.nx && smooth > a.threshold;
            const int l = y * kTile + lx;
            s_lab[l] = fg[r] ? l : -1;
            s_cnt[l] = 0;
        }
        __syncthreads();
        // every pixel joins the four neighbours before it in raster order
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) {
            if (!fg[r]) continue;
            const int y = ly + r * kRows, l = y * kTile + lx;
            if (lx > 0 && LdsOps::load(s_lab + l - 1) >= 0) join<LdsOps>(s_lab, l, l - 1);
            if (y > 0) {
                if (LdsOps::load(s_lab + l - kTile) >= 0) join<LdsOps>(s_lab, l, l - kTile);
                if (lx > 0 && LdsOps::load(s_lab + l - kTile - 1) >= 0)
                    join<LdsOps>(s_lab, l, l - kTile - 1);
                if (lx < kTile - 1 && LdsOps::load(s_lab + l - kTile + 1) >= 0)
                    join<LdsOps>(s_lab, l, l - kTile + 1);
            }
        }
        __syncthreads();
        int root[kPerThread];
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) {
            root[r] = -1;
            if (!fg[r]) continue;
            root[r] = find_root<LdsOps>(s_lab, (ly + r * kRows) * kTile + lx);
            atomicAdd(s_cnt + root[r], 1);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) {
            const int y = ly + r * kRows;
            if (y0 + y >= a.ny || x0 + lx >= a.nx) continue;
            const size_t p = (size_t)(y0 + y) * a.nx + x0 + lx;
            a.labels[p] = root[r] < 0 ? -1
                                      : (y0 + root[r] / kTile) * a.nx + x0 + root[r] % kTile;
            a.count[p] = s_cnt[y * kTile + lx];
        }
    }
}

// ---- joins across the tile borders ---------------------------------------------
// Thread t takes a pixel of a tile's first row (t < nrow_pix) or first column
// and joins it with the three pixels next to it in the row above / the column
// to the left.  Two pixels of different tiles that touch differ in their tile
// column -- then the right one is in a first column and the left one among its
// three -- or only in their tile row, likewise: every such pair is joined.
__global__ __launch_bounds__(kThreads) void k_segment_merge(int ny, int nx, int64_t nrow_pix,
                                                             int64_t total, int32_t *labels) {
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * kThreads) {
        int x, y, dxs, dys;  // the three neighbours: (x - 1 + k dxs, y - 1 + k dys), k = 0, 1, 2
        if (t < nrow_pix) {
            y = (int)(t / nx + 1) * kTile;
            x = (int)(t % nx);
            dxs = 1;
            dys = 0;
        } else {
            const int64_t u = t - nrow_pix;
            x = (int)(u / ny + 1) * kTile;
            y = (int)(u % ny);
            dxs = 0;
            dys = 1;
        }
        const int p = y * nx + x;
        if (GlobalOps::load(labels + p) < 0) continue;
        for (int k = 0; k < 3; ++k) {
            const int qx = x - 1 + k * dxs, qy = y - 1 + k * dys;
            if (qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
            const int q = qy * nx + qx;
            if (GlobalOps::load(labels + q) >= 0) join<GlobalOps>(labels, p, q);
        }
    }
}

// labels[p] = root of p; a tile-local root that is not the root hands its count
// over.  A pixel that another thread walks through points at its former parent
// or at its root, both ancestors; count[p] of such a pixel is written by nobody.
__global__ __launch_bounds__(kThreads) void k_segment_flatten(int64_t npix, int32_t *labels,
                                                               int32_t *count) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < npix;
         i += (int64_t)gridDim.x * kThreads) {
        const int p = (int)i;
        if (GlobalOps::load(labels + p) < 0) continue;
        const int root = find_root<GlobalOps>(labels, p);
        if (root == p) continue;
        __hip_atomic_store(labels + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int c = count[p];
        if (c > 0) atomicAdd(count + root, c);
    }
}

// ---- sizes and renumbering ------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_segment_roots(int64_t npix, int npixels,
                                                             const int32_t *__restrict__ labels,
                                                             const int32_t *__restrict__ count,
                                                             int32_t *__restrict__ keep) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < npix;
         i += (int64_t)gridDim.x * kThreads)
        keep[i] = labels[i] == (int32_t)i && count[i] >= npixels;
}

// rank: the inclusive prefix sum of keep.  segmap may be labels.
__global__ __launch_bounds__(kThreads) void k_segment_relabel(int64_t npix, const int32_t *labels,
                                                               const int32_t *__restrict__ keep,
                                                               const int32_t *__restrict__ rank,
                                                               int32_t *segmap) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < npix;
         i += (int64_t)gridDim.x * kThreads) {
        const int32_t l = labels[i];
        segmap[i] = (l >= 0 && l < npix && keep[l]) ? rank[l] : 0;
    }
}

// ---- peaks ------------------------------------------------------------------------
// An unsigned key in the order of the doubles, -0.0 taken as +0.0.
__device__ __forceinline__ unsigned long long key_of(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

struct PeakArgs {
    const void *planes;
    int64_t plane_stride;
    const int32_t *segmap;
    int64_t npix;
    int nseg;
    unsigned long long *keys;     // [nplanes][nseg], 0 at the start
    unsigned long long *indices;  // [nplanes][nseg], all ones at the start
    double *values;
};

// pass 0: keys = max key.  The maximum only grows, so a pixel whose key is not
// above a value read earlier need not be sent.  pass 1: the smallest index among
// the pixels whose key is the maximum; they all write the same decoded value.
template <typename T, int PASS>
__global__ __launch_bounds__(kThreads) void k_segment_peaks(PeakArgs a) {
    const T *plane = static_cast<const T *>(a.planes) + (size_t)blockIdx.y * a.plane_stride;
    const size_t row = (size_t)blockIdx.y * a.nseg;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.npix;
         i += (int64_t)gridDim.x * kThreads) {
        const int32_t s = a.segmap[i];
        if (s <= 0 || s > a.nseg) continue;
        const unsigned long long k = key_of((double)plane[i]);
        unsigned long long *best = a.keys + row + (s - 1);
        const unsigned long long seen =
            __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (PASS == 0) {
            if (k > seen) atomicMax(best, k);
        } else if (k == seen) {
            atomicMin(a.indices + row + (s - 1), (unsigned long long)i);
            a.values[row + (s - 1)] = value_of(k);
        }
    }
}

unsigned blocks_for(int64_t n) {
    return (unsigned)std::min<int64_t>((n + kThreads - 1) / kThreads, kMaxBlocks);
}

void check_plane(int ny, int nx) {
    SDP_REQUIRE(ny > 0 && nx > 0, "bad image dimensions");
    SDP_REQUIRE((int64_t)ny * nx < ((int64_t)1 << 31), "image planes of 2^31 pixels or more");
}

void check_planes(int nplanes, int ny, int nx, const void *planes, int dtype, int64_t stride) {
    check_plane(ny, nx);
    SDP_REQUIRE(nplanes > 0 && nplanes <= 65535, "bad number of planes");
    SDP_REQUIRE(dtype == SDP_HIP_F32 || dtype == SDP_HIP_F64,
                "the planes must be float32 or float64");
    SDP_REQUIRE(planes, "null pointer argument");
    SDP_REQUIRE(nplanes == 1 || stride >= (int64_t)ny * nx, "bad plane stride");
}

}  // namespace segment
}  // namespace sdp

extern "C" {

int sdp_hip_segment_label(int nchan, int ny, int nx, const void *planes, int dtype,
                          int64_t plane_stride, int ksize, const double *taps, double tap_sum,
                          double threshold, int32_t *labels, int32_t *count, int32_t *nonfinite,
                          void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::segment;
    return guarded(errbuf, errbuf_len, [&] {
        check_planes(nchan, ny, nx, planes, dtype, plane_stride);
        SDP_REQUIRE(ksize >= 1 && ksize % 2 == 1, "the smoothing kernel must have an odd size");
        SDP_REQUIRE(ksize <= kMaxK, "the smoothing kernel is larger than "
                                    "SDP_HIP_SEGMENT_KERNEL_MAX pixels a side");
        SDP_REQUIRE(taps && labels && count && nonfinite, "null pointer argument");
        SDP_REQUIRE(tap_sum > 0.0 && threshold == threshold, "bad kernel sum or threshold");
        hipStream_t st = as_stream(stream);
        TileArgs a;
        a.planes = planes;
        a.plane_stride = plane_stride;
        a.nchan = nchan;
        a.ny = ny;
        a.nx = nx;
        a.ksize = ksize;
        a.threshold = threshold;
        a.tap_sum = tap_sum;
        a.labels = labels;
        a.count = count;
        a.nonfinite = nonfinite;
        a.tiles_x = (nx + kTile - 1) / kTile;
        a.ntiles = (int64_t)a.tiles_x * ((ny + kTile - 1) / kTile);
        std::memset(a.taps, 0, sizeof(a.taps));
        std::memcpy(a.taps, taps, sizeof(double) * ksize * ksize);
        const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, kMaxBlocks);
        if (dtype == SDP_HIP_F64)
            k_segment_tiles<double><<<grid, kThreads, 0, st>>>(a);
        else
            k_segment_tiles<float><<<grid, kThreads, 0, st>>>(a);
        SDP_HIP_CHECK(hipGetLastError());
        const int64_t nrow_pix = (int64_t)((ny - 1) / kTile) * nx;
        const int64_t total = nrow_pix + (int64_t)((nx - 1) / kTile) * ny;
        if (total > 0) {
            k_segment_merge<<<blocks_for(total), kThreads, 0, st>>>(ny, nx, nrow_pix, total, labels);
            SDP_HIP_CHECK(hipGetLastError());
        }
        const int64_t npix = (int64_t)ny * nx;
        k_segment_flatten<<<blocks_for(npix), kThreads, 0, st>>>(npix, labels, count);
        SDP_HIP_CHECK(hipGetLastError());
    });
}

int sdp_hip_segment_roots(int ny, int nx, const int32_t *labels, const int32_t *count,
                          int npixels, int32_t *keep, void *stream, char *errbuf,
                          size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::segment;
    return guarded(errbuf, errbuf_len, [&] {
        check_plane(ny, nx);
        SDP_REQUIRE(labels && count && keep, "null pointer argument");
        const int64_t npix = (int64_t)ny * nx;
        k_segment_roots<<<blocks_for(npix), kThreads, 0, as_stream(stream)>>>(npix, npixels, labels,
                                                                              count, keep);
        SDP_HIP_CHECK(hipGetLastError());
    });
}

int sdp_hip_segment_relabel(int ny, int nx, const int32_t *labels, const int32_t *keep,
                            const int32_t *rank, int32_t *segmap, void *stream, char *errbuf,
                            size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::segment;
    return guarded(errbuf, errbuf_len, [&] {
        check_plane(ny, nx);
        SDP_REQUIRE(labels && keep && rank && segmap, "null pointer argument");
        const int64_t npix = (int64_t)ny * nx;
        k_segment_relabel<<<blocks_for(npix), kThreads, 0, as_stream(stream)>>>(npix, labels, keep,
                                                                                rank, segmap);
        SDP_HIP_CHECK(hipGetLastError());
    });
}

int sdp_hip_segment_peaks(int nplanes, int ny, int nx, const void *planes, int dtype,
                          int64_t plane_stride, const int32_t *segmap, int nseg, double *values,
                          int64_t *indices, void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::segment;
    return guarded(errbuf, errbuf_len, [&] {
        check_planes(nplanes, ny, nx, planes, dtype, plane_stride);
        SDP_REQUIRE(nseg >= 0, "bad number of segments");
        if (nseg == 0) return;
        SDP_REQUIRE(segmap && values && indices, "null pointer argument");
        hipStream_t st = as_stream(stream);
        const size_t n = (size_t)nplanes * nseg;
        PeakArgs a;
        a.planes = planes;
        a.plane_stride = plane_stride;
        a.segmap = segmap;
        a.npix = (int64_t)ny * nx;
        a.nseg = nseg;
        a.keys = scratch<unsigned long long>("segment_peak_keys", n);
        a.indices = reinterpret_cast<unsigned long long *>(indices);
        a.values = values;
        SDP_HIP_CHECK(hipMemsetAsync(a.keys, 0, n * sizeof(unsigned long long), st));
        SDP_HIP_CHECK(hipMemsetAsync(indices, 0xff, n * sizeof(int64_t), st));
        SDP_HIP_CHECK(hipMemsetAsync(values, 0, n * sizeof(double), st));
        const dim3 grid(blocks_for(a.npix), (unsigned)nplanes);
        if (dtype == SDP_HIP_F64) {
            k_segment_peaks<double, 0><<<grid, kThreads, 0, st>>>(a);
            k_segment_peaks<double, 1><<<grid, kThreads, 0, st>>>(a);
        } else {
            k_segment_peaks<float, 0><<<grid, kThreads, 0, st>>>(a);
            k_segment_peaks<float, 1><<<grid, kThreads, 0, st>>>(a);
        }
        SDP_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
