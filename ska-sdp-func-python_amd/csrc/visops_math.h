// Order-defining arithmetic of visops.hip, written against accessors so that
// the same text runs on the device (from LDS or global memory) and on the
// host (tests): numpy's pairwise summation and the weighted polynomial fit of
// remove_continuum_visibility.  fp64 throughout, no contraction.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SDP_HD __host__ __device__ __forceinline__
#define SDP_HD_NOINLINE __host__ __device__ __noinline__
#else
#define SDP_HD inline
#define SDP_HD_NOINLINE inline
#endif

#pragma clang fp contract(off)

namespace sdp {
namespace visops {

// ---- numpy's pairwise sum -------------------------------------------------
// numpy.sum over an axis that is the contiguous inner axis of the iteration
// (the channel axis of [.., nchan, 1] arrays: npol == 1) does not add the
// elements one by one but with pairwise_sum_DOUBLE / pairwise_sum_CDOUBLE
// (numpy/_core/src/umath/loops_utils.h.src): fewer than 8 numbers in order;
// up to 128 numbers in 8 interleaved accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) with the remainder added in order;
// more than that split at n/2 rounded down to a multiple of 8.  A complex
// sum works on its 2n floats, so each component has ACC = 4 accumulators over
// blocks of 4 complex numbers, leaves of up to 64 and a split at
// (n - n % 8) / 2.  pw_sum<8> is the real and pw_sum<4> the per-component
// complex variant; `get(i)` returns element i.
template <int ACC, class Get>
SDP_HD double pw_leaf(Get get, int64_t lo, int n) {
    if (n < ACC) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += get(lo + i);
        return res;
    }
    double r[ACC];
    for (int j = 0; j < ACC; ++j) r[j] = get(lo + j);
    int i = ACC;
    for (; i < n - (n % ACC); i += ACC)
        for (int j = 0; j < ACC; ++j) r[j] += get(lo + i + j);
    double res;
    if constexpr (ACC == 8) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    else res = (r[0] + r[1]) + (r[2] + r[3]);
    for (; i < n; ++i) res += get(lo + i);
    return res;
}

constexpr int kPwDepth = 32;

// the recursion pairwise(a, h) + pairwise(a + h, n - h) above a leaf, with its
// frames kept in arrays (out of line: it is the rare case and needs a stack)
template <int ACC, class Get>
SDP_HD_NOINLINE double pw_tree(Get get, int64_t lo0, int n0) {
    constexpr int kLeaf = ACC * 16;  // 128 reals, 64 complex numbers
    int64_t lo[kPwDepth];
    int n[kPwDepth];
    int stage[kPwDepth];
    double left[kPwDepth];
    int sp = 0;
    lo[0] = lo0;
    n[0] = n0;
    stage[0] = 0;
    double ret = 0.0;
    while (sp >= 0) {
        const int m = n[sp];
        const int h = ACC == 8 ? m / 2 - (m / 2) % 8 : (m - m % 8) / 2;
        if (stage[sp] == 0) {
            if (m <= kLeaf) {
                ret = pw_leaf<ACC>(get, lo[sp], m);
                --sp;
                continue;
            }
            stage[sp] = 1;
            lo[sp + 1] = lo[sp];
            n[sp + 1] = h;
            stage[sp + 1] = 0;
            ++sp;
        } else if (stage[sp] == 1) {
            left[sp] = ret;
            stage[sp] = 2;
            lo[sp + 1] = lo[sp] + h;
            n[sp + 1] = m - h;
            stage[sp + 1] = 0;
            ++sp;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}

template <int ACC, class Get>
SDP_HD double pw_sum(Get get, int64_t lo, int n) {
    return n <= ACC * 16 ? pw_leaf<ACC>(get, lo, n) : pw_tree<ACC>(get, lo, n);
}

// numpy.sum itself hands the inner loop at most its iterator buffer of 8192
// elements at a time and adds each part's pairwise sum to the running result.
constexpr int kNumpyBuffer = 8192;

template <int ACC, class Get>
SDP_HD double numpy_sum(Get get, int64_t lo, int n) {
    double res = 0.0;
    for (int off = 0; off < n; off += kNumpyBuffer)
        res = res + pw_sum<ACC>(get, lo + off, n - off < kNumpyBuffer ? n - off : kNumpyBuffer);
    return res;
}

// ---- weighted polynomial fit ----------------------------------------------
// Least squares fit of a polynomial of degree DEG to y(x_c) with weights w_c
// (numpy.polyfit's w squared), subtracted from y at every channel.  The
// basis is the monic polynomials orthogonal under the spectrum's own weights,
// built by the three-term recurrence (Forsythe 1957)
//   p_{k+1}(x) = (x - alpha_k) p_k(x) - beta_k p_{k-1}(x)
//   alpha_k = <x p_k, p_k> / <p_k, p_k>,  beta_k = <p_k, p_k> / <p_{k-1}, p_{k-1}>
// and coefficient k is <r_k, p_k> / <p_k, p_k> of the residual r_k left by
// the lower orders (the modified Gram-Schmidt form), so that the condition
// number of the Vandermonde matrix is never squared.
//
// Acc: x(c), w(c) the fit weight, yre(c) / yim(c), sub(c, re, im).  A spectrum
// may be shared by several lanes: each takes the channels first(), first() +
// step(), ... in ascending order and sum(v) returns the total of v over the
// spectrum's lanes, the same bits on each of them (one lane: first() = 0,
// step() = 1, sum(v) = v).  The order of every sum is fixed by step() alone.
// Returns kFitDone, or without touching y: kFitNoData when no channel has a
// non-zero weight, kFitDeficient when 1 <= n_live <= DEG.
constexpr int kMaxDegree = 5;
constexpr int kFitDone = 0, kFitNoData = 1, kFitDeficient = 2;

template <int DEG, class Acc>
SDP_HD int fit_subtract(Acc &a, int nchan) {
    const int c0 = a.first(), dc = a.step();
    int live = 0;
    for (int c = c0; c < nchan; c += dc) live += a.w(c) != 0.0 ? 1 : 0;
    live = (int)a.sum((double)live);
    if (live == 0) return kFitNoData;
    if (live <= DEG) return kFitDeficient;
    double alpha[DEG + 1], beta[DEG + 1], cre[DEG + 1], cim[DEG + 1];
    double gprev = 1.0;
#pragma unroll
    for (int k = 0; k <= DEG; ++k) {
        double g = 0.0, gx = 0.0, sre = 0.0, sim = 0.0;
        for (int c = c0; c < nchan; c += dc) {
            const double w = a.w(c);
            if (w == 0.0) continue;
            const double x = a.x(c);
            double pm = 0.0, p = 1.0, rre = a.yre(c), rim = a.yim(c);
#pragma unroll
            for (int j = 0; j < k; ++j) {
                rre -= cre[j] * p;
                rim -= cim[j] * p;
                const double pn = (x - alpha[j]) * p - beta[j] * pm;
                pm = p;
                p = pn;
            }
            const double wp = w * p;
            g += wp * p;
            gx += wp * p * x;
            sre += wp * rre;
            sim += wp * rim;
        }
        g = a.sum(g);
        gx = a.sum(gx);
        sre = a.sum(sre);
        sim = a.sum(sim);
        alpha[k] = gx / g;
        beta[k] = k ? g / gprev : 0.0;
        cre[k] = sre / g;
        cim[k] = sim / g;
        gprev = g;
    }
    for (int c = c0; c < nchan; c += dc) {
        const double x = a.x(c);
        double pm = 0.0, p = 1.0, fre = 0.0, fim = 0.0;
#pragma unroll
        for (int j = 0; j <= DEG; ++j) {
            fre += cre[j] * p;
            fim += cim[j] * p;
            const double pn = (x - alpha[j]) * p - beta[j] * pm;
            pm = p;
            p = pn;
        }
        a.sub(c, fre, fim);
    }
    return kFitDone;
}

}  // namespace visops
}  // namespace sdp
