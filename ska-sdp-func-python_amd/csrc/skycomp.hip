// Sky-component image operations for gfx950 (reference src/ska_sdp_func_python/
// sky_component/operations.py):
//   sdp_hip_skycomp_insert    insert_skycomponent (:583-668, with
//                             util/array_functions.py insert_array :134-178)
//   sdp_hip_skycomp_restore   restore_skycomponent (:671-741)
//   sdp_hip_skycomp_nearest   voronoi_decomposition's label image (:744-783)
//
// Images are [nplanes = nchan * npol, ny, nx] in C order, float64 or float32.
// insert and restore are gathers: a workgroup owns a kTileY x kTileX tile of
// pixels, a thread one pixel, and walks the tile's components -- a CSR list
// in component order made by the caller -- adding each one's term to the
// pixel's planes, which it holds in registers.  Every pixel therefore adds
// its terms in component order, one rounding to the pixel type per add as
// numpy's `+=` does, whatever the launch geometry; nothing is atomic.  The
// list's component records are staged in LDS, a chunk at a time.  fp
// contraction is off: a product and the add that follows are two roundings.
#include "sdp_common.h"

#pragma clang fp contract(off)

namespace sdp {
namespace skycomp {

constexpr int kTileX = SDP_HIP_SKYCOMP_TILE_X;
constexpr int kTileY = SDP_HIP_SKYCOMP_TILE_Y;
constexpr int kThreads = kTileX * kTileY;
constexpr int kMaxBlocks = 1 << 16;  // tiles beyond that are taken in a grid-stride loop
constexpr int kMaxPlaneBlock = 16;   // planes a thread holds in registers

static_assert(kThreads == 256 && kTileX == 32, "the kernels take lane & 31 as the tile column");

struct Tiles {
    const int64_t *ptr;   // [ntiles + 1]
    const int32_t *comp;  // [ptr[ntiles]], component order within a tile
    int64_t ntiles;
    int tiles_x;
};

template <typename T, int PB>
__device__ __forceinline__ void load_planes(const T *pix, size_t plane, int np, double (&v)[PB]) {
#pragma unroll
    for (int p = 0; p < PB; ++p)
        if (p < np) v[p] = (double)pix[p * plane];
}

template <typename T, int PB>
__device__ __forceinline__ void store_planes(T *pix, size_t plane, int np, const double (&v)[PB]) {
#pragma unroll
    for (int p = 0; p < PB; ++p)
        if (p < np) pix[p * plane] = (T)v[p];
}

// ---- insert -----------------------------------------------------------------
// Component c adds flux[c][plane] * ((ty[c][i] * tx[c][j]) / insertsum[c]) to
// the pixels (y0[c] + i, x0[c] + j) of its window, 0 <= i, j < L.  The weight
// is formed once per (pixel, component) and applied to the thread's planes.
struct InsertArgs {
    void *image;
    const int32_t *origin;  // [ncomp][2]: x0, y0
    const double *taps_y, *taps_x, *insertsum, *flux;
    int64_t ncomp;
    Tiles tiles;
    int nplanes, ny, nx, L;
};

constexpr int kInsertChunk = kThreads;

template <typename T, int PB>
__global__ __launch_bounds__(kThreads) void k_skycomp_insert(InsertArgs a) {
    __shared__ int32_t s_c[kInsertChunk], s_x0[kInsertChunk], s_y0[kInsertChunk];
    __shared__ double s_sum[kInsertChunk];
    const int lx = threadIdx.x & (kTileX - 1), ly = threadIdx.x / kTileX;
    const int p0 = blockIdx.y * PB;
    const int np = min(PB, a.nplanes - p0);
    const size_t plane = (size_t)a.ny * a.nx;
    for (int64_t tile = blockIdx.x; tile < a.tiles.ntiles; tile += gridDim.x) {
        const int64_t k0 = a.tiles.ptr[tile], k1 = a.tiles.ptr[tile + 1];
        if (k0 >= k1) continue;  // uniform over the workgroup
        const int px = (int)(tile % a.tiles.tiles_x) * kTileX + lx;
        const int py = (int)(tile / a.tiles.tiles_x) * kTileY + ly;
        const bool inside = px < a.nx && py < a.ny;
        T *pix = static_cast<T *>(a.image) + (size_t)p0 * plane + (size_t)py * a.nx + px;
        double v[PB];
        if (inside) load_planes<T, PB>(pix, plane, np, v);
        bool touched = false;
        for (int64_t kc = k0; kc < k1; kc += kInsertChunk) {
            const int n = (int)min((int64_t)kInsertChunk, k1 - kc);
            __syncthreads();
            if ((int)threadIdx.x < n) {
                int32_t c = a.tiles.comp[kc + threadIdx.x];
                const bool ok = c >= 0 && c < a.ncomp;
                if (!ok) c = 0;
                s_c[threadIdx.x] = c;
                // a window of an index outside the component list covers nothing
                s_x0[threadIdx.x] = ok ? a.origin[2 * (size_t)c] : a.nx;
                s_y0[threadIdx.x] = ok ? a.origin[2 * (size_t)c + 1] : a.ny;
                s_sum[threadIdx.x] = a.insertsum[c];
            }
            __syncthreads();
            if (!inside) continue;
            for (int k = 0; k < n; ++k) {
                const int j = px - s_x0[k], i = py - s_y0[k];
                if (i < 0 || i >= a.L || j < 0 || j >= a.L) continue;
                const size_t c = (size_t)s_c[k];
                const double w = (a.taps_y[c * a.L + i] * a.taps_x[c * a.L + j]) / s_sum[k];
                const double *f = a.flux + c * a.nplanes + p0;
#pragma unroll
                for (int p = 0; p < PB; ++p)
                    if (p < np) v[p] = (double)(T)(v[p] + f[p] * w);
                touched = true;
            }
        }
        if (inside && touched) store_planes<T, PB>(pix, plane, np, v);
    }
}

// ---- restore ----------------------------------------------------------------
// Component c adds flux[c][plane] * exp(-(a dx^2 + b dx dy + c dy^2)) with
// dx = column - x[c], dy = row - y[c] to every pixel of the tiles that list it.
struct RestoreArgs {
    void *image;
    const double *xy;  // [ncomp][2]: x, y
    const double *flux;
    int64_t ncomp;
    Tiles tiles;
    double a, b, c;
    int nplanes, ny, nx;
};

constexpr int kRestoreChunk = 64;

template <typename T, int PB>
__global__ __launch_bounds__(kThreads) void k_skycomp_restore(RestoreArgs a) {
    __shared__ double s_x[kRestoreChunk], s_y[kRestoreChunk], s_f[kRestoreChunk][PB];
    const int lx = threadIdx.x & (kTileX - 1), ly = threadIdx.x / kTileX;
    const int p0 = blockIdx.y * PB;
    const int np = min(PB, a.nplanes - p0);
    const size_t plane = (size_t)a.ny * a.nx;
    for (int64_t tile = blockIdx.x; tile < a.tiles.ntiles; tile += gridDim.x) {
        const int64_t k0 = a.tiles.ptr[tile], k1 = a.tiles.ptr[tile + 1];
        if (k0 >= k1) continue;
        const int px = (int)(tile % a.tiles.tiles_x) * kTileX + lx;
        const int py = (int)(tile / a.tiles.tiles_x) * kTileY + ly;
        const bool inside = px < a.nx && py < a.ny;
        T *pix = static_cast<T *>(a.image) + (size_t)p0 * plane + (size_t)py * a.nx + px;
        double v[PB];
        if (inside) load_planes<T, PB>(pix, plane, np, v);
        for (int64_t kc = k0; kc < k1; kc += kRestoreChunk) {
            const int n = (int)min((int64_t)kRestoreChunk, k1 - kc);
            __syncthreads();
            // records: lanes 0..n-1 the positions, then all lanes the fluxes
            for (int e = threadIdx.x; e < n * (PB + 1); e += kThreads) {
                const int k = e < n ? e : (e - n) / PB;
                const int32_t c = a.tiles.comp[kc + k];
                const bool ok = c >= 0 && c < a.ncomp;
                if (e < n) {
                    s_x[k] = ok ? a.xy[2 * (size_t)c] : 0.0;
                    s_y[k] = ok ? a.xy[2 * (size_t)c + 1] : 0.0;
                } else {
                    const int p = (e - n) % PB;
                    s_f[k][p] = (ok && p < np) ? a.flux[(size_t)c * a.nplanes + p0 + p] : 0.0;
                }
            }
            __syncthreads();
            if (!inside) continue;
            for (int k = 0; k < n; ++k) {
                const double dx = (double)px - s_x[k], dy = (double)py - s_y[k];
                const double g = exp(-(a.a * (dx * dx) + a.b * dx * dy + a.c * (dy * dy)));
#pragma unroll
                for (int p = 0; p < PB; ++p)
                    if (p < np) v[p] = (double)(T)(v[p] + s_f[k][p] * g);
            }
        }
        if (inside) store_planes<T, PB>(pix, plane, np, v);
    }
}

// ---- nearest component ------------------------------------------------------
// label[row][col] = argmin_c hypot(row - y[c], col - x[c]), the first minimum
// on ties.  hypot is evaluated only for a component whose squared distance is
// within 2^-48 (relative) of the best so far: one further away cannot have
// the strictly smaller hypot, both being accurate to an ulp.
constexpr int kNearestChunk = 512;

__global__ __launch_bounds__(kThreads) void k_skycomp_nearest(int ny, int nx, int64_t ncomp,
                                                               const double *__restrict__ xy,
                                                               int64_t *__restrict__ labels) {
    __shared__ double s_x[kNearestChunk], s_y[kNearestChunk];
    const int64_t npix = (int64_t)ny * nx;
    const int64_t nblocks = (npix + kThreads - 1) / kThreads;
    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int64_t idx = blk * kThreads + threadIdx.x;
        const double row = (double)(idx / nx), col = (double)(idx % nx);
        double best_h = 0.0, bound2 = 0.0;
        int64_t best = -1;
        for (int64_t c0 = 0; c0 < ncomp; c0 += kNearestChunk) {
            const int n = (int)min((int64_t)kNearestChunk, ncomp - c0);
            __syncthreads();
            for (int k = threadIdx.x; k < n; k += kThreads) {
                s_x[k] = xy[2 * (size_t)(c0 + k)];
                s_y[k] = xy[2 * (size_t)(c0 + k) + 1];
            }
            __syncthreads();
            for (int k = 0; k < n; ++k) {
                const double dy = row - s_y[k], dx = col - s_x[k];
                const double d2 = dy * dy + dx * dx;
                if (best >= 0 && !(d2 <= bound2)) continue;
                const double h = hypot(dy, dx);
                if (best < 0 || h < best_h) {
                    best = c0 + k;
                    best_h = h;
                    bound2 = d2 * (1.0 + 0x1p-48);
                }
            }
        }
        if (idx < npix) labels[idx] = best;
    }
}

void check_image(int nplanes, int ny, int nx, const void *image, int image_dtype) {
    SDP_REQUIRE(nplanes > 0 && ny > 0 && nx > 0, "bad image dimensions");
    SDP_REQUIRE(image_dtype == SDP_HIP_F32 || image_dtype == SDP_HIP_F64,
                "the image must be float32 or float64");
    SDP_REQUIRE(image, "null pointer argument");
}

Tiles make_tiles(int ny, int nx, const int64_t *tile_ptr, const int32_t *tile_comp) {
    SDP_REQUIRE(tile_ptr && tile_comp, "the per-tile component list is missing");
    Tiles t;
    t.ptr = tile_ptr;
    t.comp = tile_comp;
    t.tiles_x = (nx + kTileX - 1) / kTileX;
    t.ntiles = (int64_t)t.tiles_x * ((ny + kTileY - 1) / kTileY);
    return t;
}

// planes per thread: the smallest of 1, 4, 8, 16 that holds them all, else 16
// with the plane blocks on the grid's y
template <template <typename, int> class Launch, class Args>
void dispatch(const Args &a, int image_dtype, hipStream_t st) {
    const int pb = a.nplanes <= 1 ? 1 : a.nplanes <= 4 ? 4 : a.nplanes <= 8 ? 8 : kMaxPlaneBlock;
    const dim3 grid((unsigned)std::min<int64_t>(a.tiles.ntiles, kMaxBlocks),
                    (unsigned)((a.nplanes + pb - 1) / pb));
    SDP_REQUIRE(grid.y <= 65535u, "too many image planes");
    const bool f64 = image_dtype == SDP_HIP_F64;
    switch (pb) {
        case 1: f64 ? Launch<double, 1>::run(grid, a, st) : Launch<float, 1>::run(grid, a, st); break;
        case 4: f64 ? Launch<double, 4>::run(grid, a, st) : Launch<float, 4>::run(grid, a, st); break;
        case 8: f64 ? Launch<double, 8>::run(grid, a, st) : Launch<float, 8>::run(grid, a, st); break;
        default:
            f64 ? Launch<double, kMaxPlaneBlock>::run(grid, a, st)
                : Launch<float, kMaxPlaneBlock>::run(grid, a, st);
    }
}

template <typename T, int PB>
struct LaunchInsert {
    static void run(dim3 grid, const InsertArgs &a, hipStream_t st) {
        k_skycomp_insert<T, PB><<<grid, kThreads, 0, st>>>(a);
    }
};

template <typename T, int PB>
struct LaunchRestore {
    static void run(dim3 grid, const RestoreArgs &a, hipStream_t st) {
        k_skycomp_restore<T, PB><<<grid, kThreads, 0, st>>>(a);
    }
};

}  // namespace skycomp
}  // namespace sdp

extern "C" {

int sdp_hip_skycomp_insert(int nplanes, int ny, int nx, void *image, int image_dtype,
                           int64_t ncomp, int window, const int32_t *origin,
                           const double *taps_y, const double *taps_x, const double *insertsum,
                           const double *flux, const int64_t *tile_ptr, const int32_t *tile_comp,
                           void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::skycomp;
    return guarded(errbuf, errbuf_len, [&] {
        check_image(nplanes, ny, nx, image, image_dtype);
        SDP_REQUIRE(ncomp >= 0 && ncomp < ((int64_t)1 << 31), "bad component count");
        SDP_REQUIRE(window >= 1 && window < (1 << 20), "bad window length");
        if (ncomp == 0) return;
        SDP_REQUIRE(origin && taps_y && taps_x && insertsum && flux, "null pointer argument");
        InsertArgs a;
        a.image = image;
        a.origin = origin;
        a.taps_y = taps_y;
        a.taps_x = taps_x;
        a.insertsum = insertsum;
        a.flux = flux;
        a.ncomp = ncomp;
        a.tiles = make_tiles(ny, nx, tile_ptr, tile_comp);
        a.nplanes = nplanes;
        a.ny = ny;
        a.nx = nx;
        a.L = window;
        dispatch<LaunchInsert>(a, image_dtype, as_stream(stream));
        SDP_HIP_CHECK(hipGetLastError());
    });
}

int sdp_hip_skycomp_restore(int nplanes, int ny, int nx, void *image, int image_dtype,
                            int64_t ncomp, const double *xy, const double *flux, double a,
                            double b, double c, const int64_t *tile_ptr,
                            const int32_t *tile_comp, void *stream, char *errbuf,
                            size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::skycomp;
    return guarded(errbuf, errbuf_len, [&] {
        check_image(nplanes, ny, nx, image, image_dtype);
        SDP_REQUIRE(ncomp >= 0 && ncomp < ((int64_t)1 << 31), "bad component count");
        if (ncomp == 0) return;
        SDP_REQUIRE(xy && flux, "null pointer argument");
        RestoreArgs r;
        r.image = image;
        r.xy = xy;
        r.flux = flux;
        r.ncomp = ncomp;
        r.tiles = make_tiles(ny, nx, tile_ptr, tile_comp);
        r.a = a;
        r.b = b;
        r.c = c;
        r.nplanes = nplanes;
        r.ny = ny;
        r.nx = nx;
        dispatch<LaunchRestore>(r, image_dtype, as_stream(stream));
        SDP_HIP_CHECK(hipGetLastError());
    });
}

int sdp_hip_skycomp_nearest(int ny, int nx, int64_t ncomp, const double *xy, int64_t *labels,
                            void *stream, char *errbuf, size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::skycomp;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(ny > 0 && nx > 0, "bad image dimensions");
        SDP_REQUIRE(ncomp >= 1, "voronoi labels need at least one component");
        SDP_REQUIRE(xy && labels, "null pointer argument");
        const int64_t nblocks = ((int64_t)ny * nx + kThreads - 1) / kThreads;
        k_skycomp_nearest<<<(unsigned)std::min<int64_t>(nblocks, kMaxBlocks), kThreads, 0,
                            as_stream(stream)>>>(ny, nx, ncomp, xy, labels);
        SDP_HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
