// The in-LDS Stockham FFT of the fused x-FFT + w-screen kernels (wstack.hip:
// k_xfft_screen_fwd, k_screen_adj_xfft); device code only, also included by
// scripts/micro/fx_fft_check.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace sdp {
namespace wstack {

// ---- fused x-FFT + w screens (fp32 planes, power-of-two ngx) ------------
// One workgroup per image row iy.  Per plane of the batch the T row (c64,
// N = ngx points) is transformed in LDS by a Stockham mixed-radix FFT: N / 16
// threads hold 16 points each, radix-16 passes and at most one radix-2/4/8
// pass (natural-order output, no bit reversal), LDS padded by one element
// per 16 so the strided pass-0 writes are conflict-free.  The twiddles do not
// depend on the plane: each thread's w, w^2, w^4, w^8 per pass are computed
// once by sincospif (exact fractions) and the other powers by at most three
// products.  The invert screens the FFT's image columns straight from LDS
// into fp64 registers (the x-spectra are never written), the predict
// screens the image into the FFT's input in LDS (the zero-filled x-FFT input
// is never written or read).
__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// e^{SG 2 pi i m / 16} (SG = +1: backward, -1: forward), m a constant
template <int SG>
__device__ __forceinline__ float2 root16(int m) {
    constexpr float c16[16] = {1.0f,
                               0.92387953251128673848f,
                               0.70710678118654752440f,
                               0.38268343236508978178f,
                               0.0f,
                               -0.38268343236508978178f,
                               -0.70710678118654752440f,
                               -0.92387953251128673848f,
                               -1.0f,
                               -0.92387953251128673848f,
                               -0.70710678118654752440f,
                               -0.38268343236508978178f,
                               0.0f,
                               0.38268343236508978178f,
                               0.70710678118654752440f,
                               0.92387953251128673848f};
    m &= 15;
    return make_float2(c16[m], SG * c16[(m + 12) & 15]);  // sin = cos(. - pi/2)
}

// R-point DFT (R = 2, 4, 8, 16) of v[0..R) in registers, radix-2
// decimation in frequency: the result leaves bit-reversed (out[bitrev(r)] =
// v[r]); the callers index it through fx_brev
template <int R, int SG>
__device__ __forceinline__ void fx_dft(float2 *v) {
#pragma unroll
    for (int L = R; L >= 2; L >>= 1) {
        const int h = L >> 1;
#pragma unroll
        for (int s = 0; s < R; s += L) {
#pragma unroll
            for (int k = 0; k < h; ++k) {
                const float2 a = v[s + k], b = v[s + k + h];
                v[s + k] = make_float2(a.x + b.x, a.y + b.y);
                const float2 d = make_float2(a.x - b.x, a.y - b.y);
                v[s + k + h] = k == 0 ? d : cmulf(d, root16<SG>(k * (16 / L)));
            }
        }
    }
}

template <int R>
__device__ __forceinline__ constexpr int fx_brev(int r) {
    int o = 0;
    for (int b = 1, t = R >> 1; b < R; b <<= 1, t >>= 1)
        if (r & b) o |= t;
    return o;
}

__device__ __forceinline__ int fx_pad(int i) { return i + (i >> 4); }
// fx_pad(t + c), pt = fx_pad(t), c a multiple of T: for T % 16 == 0 it is
// pt + 17 c / 16 (an immediate offset from one base)
template <int T>
__device__ __forceinline__ int fx_padc(int t, int pt, int c) {
    if constexpr (T % 16 == 0) return pt + (c / 16) * 17;
    else return fx_pad(t + c);
}

// the 15 twiddles w^r, r = 1..15, from w, w^2, w^4, w^8
__device__ __forceinline__ void fx_powers(const float2 (&b)[4], float2 *w) {
    w[1] = b[0];
    w[2] = b[1];
    w[3] = cmulf(b[1], b[0]);
    w[4] = b[2];
    w[5] = cmulf(b[2], b[0]);
    w[6] = cmulf(b[2], b[1]);
    w[7] = cmulf(b[2], w[3]);
#pragma unroll
    for (int r = 1; r < 8; ++r) w[8 + r] = cmulf(b[3], w[r]);
    w[8] = b[3];
}

template <int LOGN>
struct FxShape {
    static constexpr int N = 1 << LOGN;
    static constexpr int T = N / 16;          // threads
    static constexpr int P16 = LOGN / 4;      // radix-16 passes
    static constexpr int RR = 1 << (LOGN % 4);  // last pass radix (1: none)
    static constexpr int LDS = N + N / 16;    // padded float2 elements
    // twiddle table (fx_twiddles), copied into LDS behind the data by each
    // workgroup: radix-16 pass p >= 1 at tw_off(p), w and w^4 per k < 16^p;
    // the last pass's e^{2 pi i t / N} at tw_off(P16)
    static constexpr int tw_off(int p) { return p <= 1 ? 0 : tw_off(p - 1) + 2 * (1 << (4 * (p - 1))); }
    static constexpr int TW = tw_off(P16) + T;
    static constexpr size_t lds_bytes() { return (size_t)(LDS + TW) * 8; }
};

// the transform of the row held as v[r] = X[t + r T] (pass 0's inputs) into
// buf (natural order, padded); ends with the workgroup synchronised
template <int LOGN, int SG>
__device__ __forceinline__ void fx_fft(float2 (&v)[16], float2 *buf, const float2 *__restrict__ twt,
                                       int t) {
    using S = FxShape<LOGN>;
    // pass 0 (Ns = 1): no twiddles, outputs to 16 t + r
    fx_dft<16, SG>(v);
    {
        float2 *const o = buf + 17 * t;  // fx_pad(16 t + r) = 17 t + r
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = v[fx_brev<16>(r)];
    }
    __syncthreads();
    const int pt = fx_pad(t);
    int ns = 16;
#pragma unroll
    for (int p = 1; p < S::P16; ++p) {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = buf[fx_padc<S::T>(t, pt, r * S::T)];
        __syncthreads();
        // twiddles w^r, w = e^{SG 2 pi i k / (16 Ns)}, k = t mod Ns
        const int k = t % ns, d = (t / ns) * ns * 16 + k;
        {
            // (kk opaque: the twiddles are loaded and multiplied out per
            // transform, not hoisted out of the caller's plane loop, where
            // they held ~60 VGPRs)
            int kk = k;
            asm volatile("" : "+v"(kk));
            float2 b[4], w[16];
            const float4 q0 = *reinterpret_cast<const float4 *>(twt + S::tw_off(p) + 2 * kk);
            b[0] = make_float2(q0.x, SG * q0.y);
            b[2] = make_float2(q0.z, SG * q0.w);
            b[1] = cmulf(b[0], b[0]);
            b[3] = cmulf(b[2], b[2]);
            fx_powers(b, w);
#pragma unroll
            for (int r = 1; r < 16; ++r) v[r] = cmulf(v[r], w[r]);
        }
        fx_dft<16, SG>(v);
        const int pd = fx_pad(d);  // (ns >= 16: r ns is a multiple of 16)
#pragma unroll
        for (int r = 0; r < 16; ++r) buf[pd + r * ns + ((r * ns) >> 4)] = v[fx_brev<16>(r)];
        __syncthreads();
        ns *= 16;
    }
    if constexpr (S::RR > 1) {
        // last pass, Ns = N / RR: butterfly j = t + T m reads and writes
        // X[j + r N / RR] in place (no hazard across threads)
        constexpr int RR = S::RR, NB = 16 / RR, STR = S::N / RR;
        int tt = t;
        asm volatile("" : "+v"(tt));
        const float2 l0 = twt[S::tw_off(S::P16) + tt], last = make_float2(l0.x, SG * l0.y);
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            float2 u[RR];
            // (unused, but without it the compiler addresses the LDS of 12 of the
            // fused kernels differently: kept so that this code stays what was measured)
            [[maybe_unused]] const int j = t + S::T * m;
#pragma unroll
            for (int r = 0; r < RR; ++r) u[r] = buf[fx_padc<S::T>(t, pt, S::T * m + r * STR)];
            // twiddle w_j^r of point j = t + T m: w_j = e^{SG 2 pi i j / N} = last *
            // e^{SG 2 pi i m / 16}
            const float2 wj = m == 0 ? last : cmulf(last, root16<SG>(m));
            float2 wr = wj;
#pragma unroll
            for (int r = 1; r < RR; ++r) {
                u[r] = cmulf(u[r], wr);
                if (r + 1 < RR) wr = cmulf(wr, wj);
            }
            fx_dft<RR, SG>(u);
#pragma unroll
            for (int r = 0; r < RR; ++r) buf[fx_padc<S::T>(t, pt, S::T * m + r * STR)] = u[fx_brev<RR>(r)];
        }
        __syncthreads();
    }
}

// the workgroup's LDS copy of the twiddle table (behind the data buffer)
template <int LOGN>
__device__ __forceinline__ float2 *fx_twl(float2 *fbuf, const float2 *__restrict__ twg, int t) {
    using S = FxShape<LOGN>;
    float2 *const twl = fbuf + S::LDS;
    for (int i = t; i < S::TW; i += S::T) twl[i] = twg[i];
    __syncthreads();
    return twl;
}

}  // namespace wstack
}  // namespace sdp
