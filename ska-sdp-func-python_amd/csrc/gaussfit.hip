// Batched 2-D Gaussian fits for gfx950 (reference src/ska_sdp_func_python/
// sky_component/operations.py:835-916, which runs astropy's LevMarLSQFitter on
// a Gaussian2D, one 15 x 15 window at a time): one kernel behind
//   sdp_hip_gauss_fit   params[f] = argmin_p sum_pixels (g(p) - z)^2
// for many independent windows, each read from its own plane.
//
// Model and derivatives are astropy's Gaussian2D.evaluate and fit_deriv in
// fp64, whatever the pixel type, in coordinates relative to the window's centre
// pixel (the centre is added back to the means at the end):
//   a = (cos^2 t / sx^2 + sin^2 t / sy^2) / 2
//   b = (sin 2t / sx^2 - sin 2t / sy^2) / 2
//   c = (sin^2 t / sx^2 + cos^2 t / sy^2) / 2
//   g = A exp(-(a dx^2 + b dx dy + c dy^2)),   residual r = g - z, unweighted
// with sx and sy bounded below by FLT_MIN on every evaluation, as astropy
// bounds them.  The start is the reference's: A = max z, means at the centre,
// sx = sy = 1, t = 0.
//
// Solver: Levenberg-Marquardt in the trust-region form of More (1978), the
// algorithm of MINPACK's lmder that the reference runs, on the normal
// equations.  Per trial point the wave forms N = J^T J (21 sums), J^T r (6) and
// r^T r; the step h solves (N + par D^2) h = -J^T r by a 6 x 6 Cholesky
// factorisation of the matrix scaled to unit diagonal, with par = 0 (the
// Gauss-Newton step) where that step lies within the trust region |D h| <=
// 1.1 delta, else par found by More's iteration on |D h| = delta (at most 10
// rounds).  D is the running maximum of the column norms of J, 1 for a column
// that is zero -- at the start sx = sy, so the theta column is exactly zero:
// that parameter is then left where it is and takes unit scale, as lmder does.
// Steps are accepted on actual / predicted reduction >= 1e-4 and delta and par
// updated by lmder's rules, the first delta 100 |D x| with the means of x in
// absolute pixels.  Following the reference's algorithm step for step keeps
// the fit in the reference's basin where theta is poorly determined.
//
// Stop (tighter than the reference's xtol 1e-7, ftol 1.49e-8): converged when
// delta <= 1e-12 |D x|, when actual and predicted relative reduction of the
// cost are both below 2^-52 (the cost no longer decreases), when the cost or
// the gradient is exactly zero; else at max_iter model evaluations (status 1).
//
// Mapping: one wavefront per fit, four fits per block of 256.  A lane owns 4
// of 256 pixel slots (225 live) and keeps its pixels in registers; the 28 sums
// are reduced by an xor butterfly, after which every lane holds the same bits,
// and every lane solves the 6 x 6 systems redundantly: no LDS, no atomics, no
// divergence within a wave, and no fit sees another's data, so a result is a
// function of its window alone.
#include "sdp_common.h"

#include <array>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace sdp {
namespace gaussfit {

constexpr int kWin = SDP_HIP_GAUSS_FIT_WINDOW;
constexpr int kHalf = kWin / 2;
constexpr int kLive = kWin * kWin;
constexpr int kWave = 64;
constexpr int kFitsPerBlock = 4;
constexpr int kThreads = kWave * kFitsPerBlock;
constexpr int kSlots = (kLive + kWave - 1) / kWave;  // pixel slots per lane
constexpr int kP = 6;                                // A, x, y, sx, sy, theta
constexpr int kSums = kP * (kP + 1) / 2 + kP + 1;
constexpr int kMaxFits = 1 << 24;

constexpr double kSigmaMin = FLT_MIN;  // float(numpy.finfo(numpy.float32).tiny)
constexpr double kEps = DBL_EPSILON;
constexpr double kDwarf = DBL_MIN;
constexpr double kPivot = 1e-13;  // of the unit-diagonal matrix: below, rank deficient
constexpr double kXtol = 1e-12;
constexpr double kFactor = 100.0;

static_assert(kWave * kSlots >= kLive, "every pixel needs a slot");

#if defined(__HIP_DEVICE_COMPILE__)
#define SDP_GLOBAL __attribute__((address_space(1)))
#else
#define SDP_GLOBAL
#endif

struct Sums {
    double N[kP][kP];  // J^T J, both triangles
    double g[kP];      // J^T r
    double F;          // r^T r; +inf when any sum is not finite
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// The sums at p over the lane's pixels z at (X, Y) from the window centre,
// then over the wave: the same bits in every lane.
__device__ __forceinline__ void sums_at(const double (&p)[kP], const double (&z)[kSlots],
                                        const double (&X)[kSlots], const double (&Y)[kSlots],
                                        const bool (&live)[kSlots], Sums &out) {
    const double A = p[0];
    const double sx = fmax(p[3], kSigmaMin), sy = fmax(p[4], kSigmaMin);
    double s, c;
    sincos(p[5], &s, &c);
    const double c2 = c * c, s2 = s * s, s2t = 2.0 * s * c, c2t = c * c - s * s;
    const double ix2 = 1.0 / (sx * sx), iy2 = 1.0 / (sy * sy);
    const double ix3 = ix2 / sx, iy3 = iy2 / sy;
    const double a = 0.5 * (c2 * ix2 + s2 * iy2);
    const double b = 0.5 * (s2t * ix2 - s2t * iy2);
    const double cc = 0.5 * (s2 * ix2 + c2 * iy2);
    const double dath = s * c * (iy2 - ix2);
    const double dbth = c2t * ix2 - c2t * iy2;
    double acc[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) acc[i] = 0.0;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const double dx = X[k] - p[1], dy = Y[k] - p[2];
        const double dx2 = dx * dx, dy2 = dy * dy, dxy = dx * dy;
        const double e = exp(-(a * dx2 + b * dxy + cc * dy2));
        const double g = A * e;
        double J[kP + 1];
        J[0] = e;
        J[1] = g * (2.0 * a * dx + b * dy);
        J[2] = g * (b * dx + 2.0 * cc * dy);
        J[3] = g * (c2 * ix3 * dx2 + s2t * ix3 * dxy + s2 * ix3 * dy2);
        J[4] = g * (s2 * iy3 * dx2 - s2t * iy3 * dxy + c2 * iy3 * dy2);
        J[5] = -g * (dath * dx2 + dbth * dxy - dath * dy2);
        J[6] = g - z[k];  // the residual, as a seventh column
        if (!live[k]) {
#pragma unroll
            for (int i = 0; i <= kP; ++i) J[i] = 0.0;
        }
        int n = 0;
#pragma unroll
        for (int i = 0; i <= kP; ++i)
#pragma unroll
            for (int j = i; j <= kP; ++j) acc[n++] += J[i] * J[j];
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
        acc[i] = wave_sum(acc[i]);
        finite = finite && isfinite(acc[i]);
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i <= kP; ++i)
#pragma unroll
        for (int j = i; j <= kP; ++j) {
            const double v = acc[n++];
            if (i < kP && j < kP) out.N[i][j] = out.N[j][i] = v;
            else if (i < kP) out.g[i] = v;
            else out.F = finite ? v : INFINITY;
        }
}

// Cholesky factor of M scaled to unit diagonal.  A row whose diagonal is not
// positive (a zero column of J) is taken out: identity in the factor, scale 0,
// so that the solution leaves that parameter alone.  Returns whether every
// pivot stayed above kPivot.
struct Factor {
    double L[kP][kP];
    double s[kP];
};

__device__ __forceinline__ bool factorise(const double (&M)[kP][kP], Factor &f) {
    double C[kP][kP];
    bool active[kP];
#pragma unroll
    for (int j = 0; j < kP; ++j) {
        active[j] = M[j][j] > 0.0;
        f.s[j] = active[j] ? 1.0 / sqrt(M[j][j]) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kP; ++i)
#pragma unroll
        for (int j = 0; j < kP; ++j)
            C[i][j] = active[i] && active[j] ? M[i][j] * f.s[i] * f.s[j] : (i == j ? 1.0 : 0.0);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kP; ++j) {
        double d = C[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= f.L[j][k] * f.L[j][k];
        if (!(d > kPivot)) {
            ok = false;
            d = 1.0;
        }
        f.L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < kP; ++i) {
            double v = C[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= f.L[i][k] * f.L[j][k];
            f.L[i][j] = v / f.L[j][j];
        }
    }
    return ok;
}

// x = M^-1 rhs from the factor of M
__device__ __forceinline__ void solve(const Factor &f, const double (&rhs)[kP], double (&x)[kP]) {
    double y[kP];
#pragma unroll
    for (int i = 0; i < kP; ++i) {
        double v = rhs[i] * f.s[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= f.L[i][k] * y[k];
        y[i] = v / f.L[i][i];
    }
#pragma unroll
    for (int i = kP - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < kP; ++k) v -= f.L[k][i] * x[k];
        x[i] = v / f.L[i][i];
    }
#pragma unroll
    for (int i = 0; i < kP; ++i) x[i] *= f.s[i];
}

__device__ __forceinline__ double scaled_norm(const double (&D)[kP], const double (&v)[kP]) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kP; ++i) t += (D[i] * v[i]) * (D[i] * v[i]);
    return sqrt(t);
}

// q^T M^-1 q for q = D^2 h / |D h|: minus the slope of |D h(par)| over |D h|
__device__ __forceinline__ double secular_slope(const Factor &f, const double (&D)[kP],
                                                const double (&h)[kP], double dxnorm) {
    double q[kP], w[kP];
#pragma unroll
    for (int i = 0; i < kP; ++i) q[i] = D[i] * D[i] * h[i] / dxnorm;
    solve(f, q, w);
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kP; ++i) t += q[i] * w[i];
    return t;
}

// The step h with (N + par D^2) h = -g and |D h| within a tenth of delta, or
// the Gauss-Newton step (par = 0) where it is no longer than that; returns
// |D h| and updates par.
__device__ __forceinline__ double lm_step(const Sums &S, const double (&D)[kP], double delta,
                                          double &par, double (&h)[kP]) {
    double mg[kP];
#pragma unroll
    for (int i = 0; i < kP; ++i) mg[i] = -S.g[i];
    Factor f;
    const bool nonsingular = factorise(S.N, f);
    solve(f, mg, h);
    double dxnorm = scaled_norm(D, h);
    double fp = dxnorm - delta;
    if (nonsingular && fp <= 0.1 * delta) {
        par = 0.0;
        return dxnorm;
    }
    double gs = 0.0;
#pragma unroll
    for (int i = 0; i < kP; ++i) gs += (S.g[i] / D[i]) * (S.g[i] / D[i]);
    const double gnorm = sqrt(gs);
    double paru = gnorm / delta;
    if (paru == 0.0) paru = kDwarf / fmin(delta, 0.1);
    double parl = 0.0;
    if (nonsingular) parl = fp / (delta * secular_slope(f, D, h, dxnorm));
    par = fmin(fmax(par, parl), paru);
    if (par == 0.0) par = dxnorm > 0.0 ? gnorm / dxnorm : 0.0;
    for (int it = 1; it <= 10; ++it) {
        if (par == 0.0) par = fmax(kDwarf, 0.001 * paru);
        double M[kP][kP];
#pragma unroll
        for (int i = 0; i < kP; ++i)
#pragma unroll
            for (int j = 0; j < kP; ++j) M[i][j] = S.N[i][j] + (i == j ? par * D[i] * D[i] : 0.0);
        factorise(M, f);
        solve(f, mg, h);
        dxnorm = scaled_norm(D, h);
        const double before = fp;
        fp = dxnorm - delta;
        if (fabs(fp) <= 0.1 * delta || (parl == 0.0 && fp <= before && before < 0.0) || it == 10)
            break;
        const double parc = fp / (delta * secular_slope(f, D, h, dxnorm));
        if (fp > 0.0) parl = fmax(parl, par);
        if (fp < 0.0) paru = fmin(paru, par);
        par = fmax(parl, par + parc);
    }
    return dxnorm;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_gauss_fit(int nfit, const void *const *planes,
                                                        const int64_t *row_strides,
                                                        const int32_t *x0s, const int32_t *y0s,
                                                        int max_iter, double *__restrict__ params,
                                                        int32_t *__restrict__ status,
                                                        int32_t *__restrict__ niter) {
    const int lane = (int)threadIdx.x % kWave;
    const int fit = (int)blockIdx.x * kFitsPerBlock + (int)threadIdx.x / kWave;
    if (fit >= nfit) return;  // the whole wave
    const SDP_GLOBAL T *plane = (const SDP_GLOBAL T *)static_cast<const T *>(planes[fit]);
    const int64_t stride = row_strides[fit];
    const int x0 = x0s[fit], y0 = y0s[fit];

    double z[kSlots], X[kSlots], Y[kSlots];
    bool live[kSlots];
    bool bad = false;
    double zmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int slot = lane + kWave * k;
        live[k] = slot < kLive;
        const int row = live[k] ? slot / kWin : 0, col = live[k] ? slot % kWin : 0;
        z[k] = live[k] ? (double)plane[(int64_t)(y0 + row) * stride + (x0 + col)] : 0.0;
        X[k] = (double)(col - kHalf);
        Y[k] = (double)(row - kHalf);
        bad = bad || !isfinite(z[k]);
        if (live[k]) zmax = fmax(zmax, z[k]);
    }
    bad = __any(bad);
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) zmax = fmax(zmax, __shfl_xor(zmax, m, kWave));

    const double off[kP] = {0.0, (double)(x0 + kHalf), (double)(y0 + kHalf), 0.0, 0.0, 0.0};
    double p[kP] = {zmax, 0.0, 0.0, 1.0, 1.0, 0.0};
    double D[kP], xabs[kP];
    Sums S;
    int state = 1, nfev = 0;
    if (!bad) {
        sums_at(p, z, X, Y, live, S);
        nfev = 1;
        bad = !isfinite(S.F);
    }
    if (!bad) {
#pragma unroll
        for (int i = 0; i < kP; ++i) {
            D[i] = sqrt(S.N[i][i]);
            if (D[i] == 0.0) D[i] = 1.0;
            xabs[i] = p[i] + off[i];
        }
        double xnorm = scaled_norm(D, xabs);
        double delta = xnorm > 0.0 ? kFactor * xnorm : kFactor;
        double par = 0.0;
        bool first = true;
        while (nfev < max_iter) {
            bool any_g = false;
#pragma unroll
            for (int i = 0; i < kP; ++i) any_g = any_g || S.g[i] != 0.0;
            if (S.F == 0.0 || !any_g) {
                state = 0;
                break;
            }
            double h[kP], pn[kP];
            const double pnorm = lm_step(S, D, delta, par, h);
#pragma unroll
            for (int i = 0; i < kP; ++i) pn[i] = p[i] + h[i];
            Sums Sn;
            sums_at(pn, z, X, Y, live, Sn);
            ++nfev;
            if (first) {
                delta = fmin(delta, pnorm);
                first = false;
            }
            // the reductions of the cost relative to it: actual, and predicted by
            // the linear model; norms as square roots, as lmder has them
            const double fnorm = sqrt(S.F), fnorm1 = sqrt(Sn.F);
            const double actred = 0.1 * fnorm1 < fnorm ? 1.0 - (fnorm1 / fnorm) * (fnorm1 / fnorm)
                                                       : -1.0;
            double hNh = 0.0;
#pragma unroll
            for (int i = 0; i < kP; ++i) {
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < kP; ++j) t += S.N[i][j] * h[j];
                hNh += h[i] * t;
            }
            const double t1 = fmax(hNh, 0.0) / S.F;
            const double t2 = par * pnorm * pnorm / S.F;
            const double prered = t1 + 2.0 * t2;
            const double dirder = -(t1 + t2);
            const double ratio = prered != 0.0 ? actred / prered : 0.0;
            if (ratio <= 0.25) {
                double temp = actred >= 0.0 ? 0.5 : 0.5 * dirder / (dirder + 0.5 * actred);
                if (0.1 * fnorm1 >= fnorm || temp < 0.1) temp = 0.1;
                delta = temp * fmin(delta, pnorm / 0.1);
                par /= temp;
            } else if (par == 0.0 || ratio >= 0.75) {
                delta = pnorm / 0.5;
                par *= 0.5;
            }
            if (ratio >= 1e-4) {
#pragma unroll
                for (int i = 0; i < kP; ++i) {
                    p[i] = pn[i];
                    xabs[i] = p[i] + off[i];
                }
                S = Sn;
                xnorm = scaled_norm(D, xabs);
#pragma unroll
                for (int i = 0; i < kP; ++i) D[i] = fmax(D[i], sqrt(S.N[i][i]));
            }
            if ((fabs(actred) <= kEps && prered <= kEps && 0.5 * ratio <= 1.0) ||
                delta <= kXtol * xnorm) {
                state = 0;
                break;
            }
            if (!isfinite(delta) || !isfinite(par)) {
                bad = true;
                break;
            }
        }
    }
    if (lane < kP) {
        double v = p[lane] + off[lane];
        if (lane == 3 || lane == 4) v = fmax(v, kSigmaMin);
        params[(int64_t)fit * kP + lane] = bad ? NAN : v;
    }
    if (lane == 0) {
        status[fit] = bad ? 2 : state;
        if (niter) niter[fit] = nfev;
    }
}

// The tables of a call: written to pinned host memory, copied to the device
// buffer of the same slot on the call's stream.  A slot is reused only after
// the event recorded behind its last call has completed, so calls may be in
// flight on several streams without a synchronisation here.
constexpr int kTableSlots = 4;

struct Slot {
    void *host = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
};

struct Slots {
    std::array<Slot, kTableSlots> slot;
    int next = 0;
};

std::mutex g_mu;
std::map<int, Slots> g_slots;

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace gaussfit
}  // namespace sdp

extern "C" {

int sdp_hip_gauss_fit(int nfit, const void *const *planes, int dtype, const int64_t *row_strides,
                      const int32_t *x0, const int32_t *y0, int max_iter, double *params,
                      int32_t *status, int32_t *niter, void *stream, char *errbuf,
                      size_t errbuf_len) {
    using namespace sdp;
    using namespace sdp::gaussfit;
    return guarded(errbuf, errbuf_len, [&] {
        SDP_REQUIRE(dtype == SDP_HIP_F32 || dtype == SDP_HIP_F64,
                    "the planes must be float32 or float64");
        SDP_REQUIRE(nfit >= 0 && nfit <= kMaxFits,
                    "gauss_fit takes 0 .. " + std::to_string(kMaxFits) + " fits per call");
        SDP_REQUIRE(max_iter >= 1, "max_iter must be at least 1");
        if (nfit == 0) return;
        SDP_REQUIRE(planes && row_strides && x0 && y0 && params && status, "null pointer argument");
        const size_t esize = dtype == SDP_HIP_F64 ? 8 : 4;
        for (int f = 0; f < nfit; ++f) {
            SDP_REQUIRE(planes[f] && reinterpret_cast<uintptr_t>(planes[f]) % esize == 0,
                        "a plane pointer is null or not aligned to its element");
            SDP_REQUIRE(row_strides[f] >= 0, "a row stride is negative");
            SDP_REQUIRE(x0[f] >= 0 && y0[f] >= 0 && x0[f] <= INT32_MAX - kWin &&
                            y0[f] <= INT32_MAX - kWin,
                        "a window starts off its plane");
        }
        const size_t n = (size_t)nfit;
        const size_t off_rs = round16(n * sizeof(void *));
        const size_t off_x0 = off_rs + round16(n * sizeof(int64_t));
        const size_t off_y0 = off_x0 + round16(n * sizeof(int32_t));
        const size_t bytes = off_y0 + round16(n * sizeof(int32_t));

        const hipStream_t st = as_stream(stream);
        int dev = 0;
        SDP_HIP_CHECK(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_mu);
        Slots &ss = g_slots[dev];
        const int idx = ss.next;
        ss.next = (ss.next + 1) % kTableSlots;
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
        std::memcpy(h, planes, n * sizeof(void *));
        std::memcpy(h + off_rs, row_strides, n * sizeof(int64_t));
        std::memcpy(h + off_x0, x0, n * sizeof(int32_t));
        std::memcpy(h + off_y0, y0, n * sizeof(int32_t));

        char *d = scratch<char>("gauss_fit_tables" + std::to_string(idx), bytes);
        SDP_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
        const auto d_planes = reinterpret_cast<const void *const *>(d);
        const auto d_rs = reinterpret_cast<const int64_t *>(d + off_rs);
        const auto d_x0 = reinterpret_cast<const int32_t *>(d + off_x0);
        const auto d_y0 = reinterpret_cast<const int32_t *>(d + off_y0);
        const unsigned blocks = (unsigned)((nfit + kFitsPerBlock - 1) / kFitsPerBlock);
        if (dtype == SDP_HIP_F64)
            k_gauss_fit<double><<<blocks, kThreads, 0, st>>>(nfit, d_planes, d_rs, d_x0, d_y0,
                                                             max_iter, params, status, niter);
        else
            k_gauss_fit<float><<<blocks, kThreads, 0, st>>>(nfit, d_planes, d_rs, d_x0, d_y0,
                                                            max_iter, params, status, niter);
        SDP_HIP_CHECK(hipGetLastError());
        SDP_HIP_CHECK(hipEventRecord(s.done, st));
    });
}

}  // extern "C"
