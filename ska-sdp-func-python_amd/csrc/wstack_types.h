// w-stacking NUFFT, stage 0: what every other stage shares.  The constants,
// the call geometry `Geo` (built by plan_geometry_once and passed by value to
// every kernel), the record and work-item layouts (VisRec, RecC, Item,
// FineItem), the ES kernel and its Phi lookup, and the fp64 coordinates of a
// visibility (vis_coord_v) with the bucket keys made from them (coord_key:
// single-level and coarse plans; tiled_key: g.tiled).
// Read first: Geo, then vis_coord_v.  Geo::fold (the invert's Hermitian fold)
// is applied in vis_coord_v.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

namespace sdp {
namespace wstack {

constexpr double kCLight = 299792458.0;
constexpr int kTileCoarse = 16;  // bucket edge (cells) of large grids (sub-sorted by cell)
// one-cell buckets ordered x-pair major (key tile = ((ic >> 1) * ngy + jc) *
// 2 + (ic & 1)), so a bucket's records share their footprint origin and 16
// consecutive buckets form one 2 x 8-cell work-item region
constexpr int kTileCell = 1;
constexpr int kGroupCell = 16;
constexpr int64_t kMaxCellKeys = (int64_t)1 << 28;
constexpr int kGridAlign = 16;   // padded grid edges are multiples of this
constexpr int kChunkMin = 1024;   // records per work item: chosen per call in
constexpr int kChunkMax = 8192;   // [kChunkMin, kChunkMax] (chunk_size())
constexpr int kMaxW = 8;
constexpr int kPhiTab = 8193;  // Phi(xi) table on xi in [0, 0.5]
constexpr int kFftBatchMax = 16;                      // planes per FFT batch
constexpr size_t kFftBatchBytes = (size_t)16 << 30;  // y-spectra buffers per batch

struct Geo {
    int W;
    float beta, inv_half_w, beta_l2e;
    int nx, ny, ngx, ngy;
    double px, py;
    int do_w, nplanes, nps;  // nps = number of distinct first planes
    double w0, dw, s0;
    int sub, nty, ntiles;  // bucket edge in cells, buckets per window column, buckets
    // bucket window: the footprint origins of all visibilities lie in cells
    // [wx0, wx0 + wnx) x [wy0, wy0 + wny) (16-aligned), so only the window's
    // buckets are histogrammed, scanned and itemised
    int wx0, wy0, wnx, wny;
    int grp;               // consecutive buckets (along y) per work-item group
    // keys per bucket (16x16-cell buckets: a power of 2 > 1): the count pass
    // spreads a bucket's histogram counter over `salt` adjacent counters by
    // row, so the uv core's hot buckets take several memory-side atomic
    // streams; the sub-buckets are adjacent, so the bucket stays contiguous
    int salt;
    double su;  // sign applied to u and w (-1 with SDP_HIP_FLIP_UW)
    int nchan;
    int64_t nrow;
    // one-cell keys: blocks of bx x 8 cells (bx = 2, 4 or 8; bxs = log2 bx),
    // each bx / 2 groups of 2 x 8 cells, consecutive in the key order
    int bx, bxs;
    // w slab (SDP_HIP_W_SLAB): this call grids only the visibilities whose
    // first plane lies in [slab_lo, slab_lo + nps) of the sequence's layout of
    // nps_all first planes; w0 is then the slab's first plane, and the others
    // are skipped without being counted as out of bounds
    int slab, slab_lo, nps_all;
    // two-level bucketing of one-cell keys (tiled = 1): the window is cut into
    // tlx x tly bins of 64 x 64 cells per first plane (nbins in all); the
    // keys of a bin are contiguous (bin-major, 4096 per bin)
    int tiled, tlx, tly, nbins;
    double inv_nchan;  // 1 / nchan (the two-level passes' row = v / nchan)
    // folded per-visibility factors (geo_factors): a = u_m s kax, b = v_m s
    // kby, fractional plane pw = w_m s kpw - kpw0 of the FULL layout (a w
    // slab subtracts its first plane as an integer, so slabs partition the
    // visibilities exactly) -- no fp64 division per visibility
    double kax, kby, kpw, kpw0;
    // Hermitian fold (invert only, plan_geometry): a visibility with
    // su * u < 0 is gridded at (-u, -v, -w) with its value conjugated -- the
    // same real part of the image -- so every footprint lies in the grid rows
    // from ngx / 2 - W / 2 - 1 up and the plane passes run over half the band.
    // The plane layout (w0, dw, nplanes, nps) is that of the unfolded w range.
    int fold;
};

struct __attribute__((aligned(32))) VisRec {
    float cre, cim;    // gridding: vis*wgt*exp(2 pi i w s0); degridding: wgt*exp(-2 pi i w s0)
    float fu, fv, fw;  // offset of the first tap from the exact position (cells/planes)
    uint32_t ij;       // footprint start in the centred grid: ic0 | jc0 << 16
    uint32_t p0;       // first w plane
    uint32_t idx;      // row * nchan + chan
};
static_assert(sizeof(VisRec) == 32, "record layout");

// 16-byte record of the 4-padded invert (k_grid_mfma_pad): the value and the
// footprint offsets as fixed-point fractions, e = (1 - W/2) - f in [0, 1):
// u in lo[0:21), v in lo[21:32) | hi[0:10), w in hi[10:32) (steps of 2^-21,
// 2^-21, 2^-22 cells / planes, i.e. rounding errors <= 2.4e-7 / 1.2e-7 --
// fp32 offsets near 3.5 round to 1.2e-7).  The cell and the first plane are
// those of the record's bucket, so the record does not carry them.
struct __attribute__((aligned(16))) RecC {
    float cre, cim;
    uint32_t lo, hi;
};
static_assert(sizeof(RecC) == 16, "record layout");

__device__ __forceinline__ uint32_t fix_frac(double e, int bits) {
    const double q = floor(e * (double)(1u << bits) + 0.5);
    return (uint32_t)fmin(fmax(q, 0.0), (double)((1u << bits) - 1u));
}

struct Item {
    uint32_t b, e, tile, p0;
};

// Large grids (16x16-cell buckets): work item of one group of 4 2x2-cell
// buckets (a 2 x 8-cell region) inside a sub-sorted coarse item; records
// [b, e) ordered by bucket, bucket j of the group ending at o[j] (k_subsort)
struct FineItem {
    uint32_t b, e, tile, p0;
    uint32_t o[16];  // end of bucket j of the group (2x2 buckets: j < 4; cells: j < 16)
};

// ------------------------------------------------------------------------
// helpers: environment knobs (host), then the device side -- ES kernel, Phi
// lookup, visibility coordinates and bucket keys
// ------------------------------------------------------------------------
static int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

// ES kernel exp(beta (sqrt(1 - x^2) - 1)), x = 2t/W; `beta_l2e` = beta*log2(e)
// so the raw v_exp_f32 (2^x) and v_sqrt_f32 are used directly.
__device__ __forceinline__ float es_kernel(float t, float inv_half_w, float beta_l2e) {
    const float x = t * inv_half_w;
    const float y = 1.0f - x * x;
    const float e =
        __builtin_amdgcn_exp2f(beta_l2e * (__builtin_amdgcn_sqrtf(fmaxf(y, 0.0f)) - 1.0f));
    return y > 0.0f ? e : 0.0f;
}

// 4-point Lagrange interpolation of the tabulated Phi on [0, 0.5].
__device__ __forceinline__ double phi_lookup(const double *__restrict__ tab, double xi) {
    xi = fabs(xi);
    const double t = xi * (2.0 * (kPhiTab - 1));
    int k = (int)t;
    k = min(max(k, 1), kPhiTab - 3);
    const double f = t - k;
    const double p0 = tab[k - 1], p1 = tab[k], p2 = tab[k + 1], p3 = tab[k + 2];
    const double fm1 = f + 1.0, f1 = f - 1.0, f2 = f - 2.0;
    return -p0 * f * f1 * f2 / 6.0 + p1 * fm1 * f1 * f2 / 2.0 - p2 * fm1 * f * f2 / 2.0 +
           p3 * fm1 * f * f1 / 6.0;
}

struct Coord {
    int ic0, jc0, p0;
    float fu, fv, fw;
    double du, dv, dw;  // the same offsets in fp64 (RecC encoding)
    double w;  // w in wavelengths (sign applied)
    bool ok;
    bool skip = false;  // w slab: inside the sequence's layout, outside this slab
    bool conj = false;  // folded (Geo::fold): the record holds the value's conjugate
};

// the visibility's grid coordinates from its row's uvw (metres) and its
// frequency
__device__ __forceinline__ Coord vis_coord_v(const Geo &g, double um, double vm, double wm,
                                             double s) {
    Coord c;
    double ws = wm * s;
    // (the ORIGINAL w: the writers rotate by the original coordinates' phase
    // and conjugate the rotated value)
    c.w = g.su * ws;
    double a = (um * s) * g.kax;
    double b = (vm * s) * g.kby;
    // the fold's one predicate (k_bounds uses the same): u = 0 does not fold
    if (g.fold && g.su * um < 0.0) {
        a = -a;
        b = -b;
        ws = -ws;
        c.conj = true;
    }
    c.ok = fabs(a) < (double)g.ngx && fabs(b) < (double)g.ngy;
    if (!c.ok) return c;
    const double fa = floor(a - 0.5 * g.W), fb = floor(b - 0.5 * g.W);
    c.du = fa + 1.0 - a;
    c.dv = fb + 1.0 - b;
    c.fu = (float)c.du;
    c.fv = (float)c.dv;
    // (fa + 1 + ng/2) mod ng: |a| < ng puts it in (-ng, 2 ng), so one
    // conditional add or subtract is the modulo (no integer division)
    int ic = (int)fa + 1 + g.ngx / 2, jc = (int)fb + 1 + g.ngy / 2;
    ic = ic >= g.ngx ? ic - g.ngx : (ic < 0 ? ic + g.ngx : ic);
    jc = jc >= g.ngy ? jc - g.ngy : (jc < 0 ? jc + g.ngy : jc);
    c.ic0 = ic;
    c.jc0 = jc;
    // the footprint origin must lie in the bucket window and the first plane
    // in [0, nps): always so when the geometry comes from these
    // visibilities' own extremes (a margin of >= 2 cells / half a plane), but
    // a batch of a batched invert is checked against the bounds its caller
    // gave (out of them it would index outside the histogram or the planes)
    c.ok = (unsigned)(c.ic0 - g.wx0) < (unsigned)g.wnx &&
           (unsigned)(c.jc0 - g.wy0) < (unsigned)g.wny;
    if (g.do_w) {
        const double pw = fma(ws, g.kpw, -g.kpw0);
        const double fp = floor(fmin(fmax(pw - 0.5 * g.W, -2.0), 2.0e9));
        c.dw = fp + 1.0 - pw;
        c.fw = (float)c.dw;
        c.p0 = (int)fp + 1 - g.slab_lo;
        const bool in_slab = c.p0 >= 0 && c.p0 < g.nps;
        c.ok = c.ok && in_slab;
        if (g.slab) c.skip = !in_slab && (unsigned)(c.p0 + g.slab_lo) < (unsigned)g.nps_all;
        c.p0 = min(max(c.p0, 0), g.nps - 1);
    } else {
        c.p0 = 0;
        c.fw = 0.0f;
        c.dw = 0.0;
    }
    return c;
}

__device__ __forceinline__ Coord vis_coord(const Geo &g, const double *__restrict__ uvw,
                                           int64_t rs, int64_t row, double f) {
    return vis_coord_v(g, uvw[row * rs], uvw[row * rs + 1], uvw[row * rs + 2], f / kCLight);
}

// w slab: the visibility's first plane (computed exactly as vis_coord does)
// lies in the sequence's layout but outside this call's slab -- tested before
// anything else of the visibility is read
__device__ __forceinline__ bool slab_out_v(const Geo &g, double wm, double s) {
    const double pw = fma(wm * s, g.kpw, -g.kpw0);
    const int p0 = (int)floor(fmin(fmax(pw - 0.5 * g.W, -2.0), 2.0e9)) + 1 - g.slab_lo;
    return (p0 < 0 || p0 >= g.nps) && (unsigned)(p0 + g.slab_lo) < (unsigned)g.nps_all;
}

__device__ __forceinline__ bool slab_out(const Geo &g, const double *__restrict__ uvw, int64_t rs,
                                         int64_t row, double f) {
    return slab_out_v(g, uvw[row * rs + 2], f / kCLight);
}

// p0-major bucket keys: the items of a range of first planes are contiguous.
// One-cell keys inside a plane: block (x-major), x pair in the block, y, x
// parity -- 16 consecutive keys are a group of 2 x 8 cells.
// Two-level (tiled) one-cell keys: bin = (first plane, 64 x 64-cell tile of
// the window), then inside the bin: x pair (32), y block of 8 (8), and the
// cell of the 2 x 8-cell group, (y & 7) * 2 + (x & 1) -- 16 consecutive keys
// are again one group, 256 groups per bin.
constexpr int kTile = 64;
constexpr int kBinCells = kTile * kTile;
__device__ __forceinline__ unsigned tiled_key(const Geo &g, const Coord &c) {
    const int ic = c.ic0 - g.wx0, jc = c.jc0 - g.wy0;
    const int tile = (ic >> 6) * g.tly + (jc >> 6);
    const int lx = ic & 63, ly = jc & 63;
    const unsigned local = ((unsigned)(((lx >> 1) << 3) | (ly >> 3)) << 4) |
                           (unsigned)((ly & 7) << 1) | (unsigned)(lx & 1);
    return ((unsigned)c.p0 * (unsigned)(g.tlx * g.tly) + (unsigned)tile) * (unsigned)kBinCells +
           local;
}

__device__ __forceinline__ unsigned coord_key(const Geo &g, const Coord &c, int64_t row) {
    if (g.tiled) return tiled_key(g, c);
    const int ic = c.ic0 - g.wx0, jc = c.jc0 - g.wy0;
    const int tile =
        g.sub == kTileCell
            ? ((((ic >> g.bxs) * (g.wny >> 3) + (jc >> 3)) << (g.bxs - 1)) + ((ic & (g.bx - 1)) >> 1)) *
                      16 + (jc & 7) * 2 + (ic & 1)
            : (ic / g.sub) * g.nty + (jc / g.sub);
    return ((unsigned)c.p0 * (unsigned)g.ntiles + (unsigned)tile) * (unsigned)g.salt +
           ((unsigned)row & (unsigned)(g.salt - 1));
}

}  // namespace wstack
}  // namespace sdp
