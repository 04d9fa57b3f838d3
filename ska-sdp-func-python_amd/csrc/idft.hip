// Inverse sky-component DFT for gfx950: sdp_hip_idft_point_v00 and
// sdp_hip_idft_point_metres, the adjoint of dft.hip (reference
// src/ska_sdp_func_python/imaging/dft.py:340-387, the sums of :365-371):
//
//   S[c, chan, pol] = sum_row w (1 - flag) V[row, chan, pol] exp(+2 pi i (u l_c + v m_c + w (n_c - 1)))
//   W[chan, pol]    = sum_row w (1 - flag)
//
// Both unnormalised: the division S / W is the caller's, so a row-sharded
// caller can all-reduce S and W first.
//
// The phase is dft.hip's: one v_mfma_f64_16x16x4_f64 of 16 rows' uvw_lambda
// with 16 components' (l, m, n - 1, 0), reduced to turns in fp64
// (v_fract_f64).  Lane l of the product holds component l & 15 against rows
// (l >> 4) + 4 i, so the adjoint's sum over rows stays in the lane's own
// registers (the forward kernel needs a 16-lane butterfly per output).
//
// Work split: grid = (row partition, component chunk, channel).  A workgroup
// stages 64 TPW rows (uvw_lambda and x = w (1 - flag) V) through LDS; each of
// its 4 waves takes TPW of the stage's 16-row tiles against the same CC =
// 8 / npol component tiles (128 / npol components), whose accumulators live
// in registers.  TPW = 8 (512 rows) for complex64 and 4 (256 rows) for
// complex128 visibilities: staging, the two barriers and the fp64 flush are
// per stage, a quarter of the complex64 inner loop's instructions at 256
// rows.  A row partition strides over the stages (partition p takes stages
// p, p + P, ...), P capped so that the grid is about kTargetWgs workgroups
// whatever nrow is.  The partition is the fastest grid index and P
// a multiple of 8: consecutive workgroups go to the 8 XCDs in turn, so the
// workgroups that read the same rows for different component chunks share an
// XCD and its L2 (a speed choice only; nothing depends on the placement).
//
// Accumulation: complex128 visibilities use fp64 sincospi, products and sums.
// complex64 visibilities use v_sin_f32 / v_cos_f32 and fp32 products; their
// fp32 partial sums are bounded to one stage of one lane, 8 tiles x 4 rows =
// 32 terms, and are then added into fp64 accumulators, so no fp32 chain is
// longer than 32 terms whatever nrow is.
//
// Reduction: no atomics.  The lane groups of a wave are summed by two fixed
// shuffles, the 4 waves through LDS in wave order, and the workgroup writes
// its partial S to scratch [partition][chan][padded comp][pol]; k_idft_reduce
// sums the partitions in index order.  W is summed in fp64 by the workgroups
// of component chunk 0 (each thread over the rows it stages, then a fixed LDS
// tree) and reduced by the same second kernel.  Two calls with the same
// inputs give the same bits.
#include <type_traits>

#include "sdp_common.h"

namespace sdp {
namespace idft {

constexpr double kCLight = 299792458.0;
constexpr int kThreads = 256;
template <class VT>
constexpr int tiles_per_wave() {  // 16-row tiles of a stage per wave
    return std::is_same<VT, double2>::value ? 4 : 8;
}
constexpr int kTargetWgs = 2048;   // workgroups aimed at: 2 rounds of 4 per CU on 256 CUs
constexpr int kMaxParts = 4096;    // row partitions at most (scratch bound)

typedef double doublex4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double keep_of(const void *flags, int bytes, int64_t i) {
    if (!bytes) return 1.0;
    double f;
    if (bytes == 8) f = (double)static_cast<const int64_t *>(flags)[i];
    else if (bytes == 4) f = (double)static_cast<const int32_t *>(flags)[i];
    else f = (double)static_cast<const int8_t *>(flags)[i];
    return 1.0 - f;
}

// VT: the visibilities' type (float2: fp32 sincos and products; double2: fp64).
// CC: component tiles of 16 per workgroup.
template <int NPOL, class VT, bool kMetres, int CC>
__global__ __launch_bounds__(kThreads) void k_idft_mfma(
    int ncomp, const double *__restrict__ dc, int64_t nrow, int nchan,
    const double *__restrict__ uvw, const double *__restrict__ freq, const VT *__restrict__ vis,
    const double *__restrict__ weight, const void *__restrict__ flags, int fbytes, int nparts,
    int ncomp_pad, double2 *__restrict__ part_s, double *__restrict__ part_w) {
    constexpr bool kF64 = std::is_same<VT, double2>::value;
    using FT = typename std::conditional<kF64, double, float>::type;
    constexpr int kChunk = CC * 16;  // components per workgroup
    constexpr int G = CC < 4 ? CC : 4;  // MFMAs issued together
    constexpr int TPW = tiles_per_wave<VT>();
    constexpr int kStage = 4 * TPW * 16;  // rows staged per pass
    __shared__ double s_a[kStage * 4];          // (u, v, w, 0) in wavelengths per staged row
    __shared__ VT s_x[kStage * NPOL];           // w (1 - flag) V per staged row
    __shared__ double2 s_fold[4 * kChunk * NPOL];  // the waves' sums; also W's tree (>= 256 NPOL doubles)
    static_assert(4 * kChunk * NPOL * 2 >= kThreads * NPOL, "W tree fits the fold buffer");

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = lane >> 4, r16 = lane & 15;
    const int part = blockIdx.x, chunk = blockIdx.y, chan = blockIdx.z;
    const int c0 = chunk * kChunk;
    const bool do_w = part_w != nullptr && chunk == 0;
    const double s = kMetres ? freq[chan] / kCLight : 1.0;

    // B operands: coordinate k of component c0 + 16 cc + r16 (padded: 0)
    double bop[CC];
#pragma unroll
    for (int cc = 0; cc < CC; ++cc) {
        const int c = c0 + 16 * cc + r16;
        bop[cc] = (c < ncomp && k < 3) ? dc[(int64_t)c * 3 + k] : 0.0;
    }
    double sr[CC][NPOL], si[CC][NPOL];  // fp64 sums over this lane's rows
#pragma unroll
    for (int cc = 0; cc < CC; ++cc)
#pragma unroll
        for (int p = 0; p < NPOL; ++p) sr[cc][p] = si[cc][p] = 0.0;
    double wsum[NPOL];
#pragma unroll
    for (int p = 0; p < NPOL; ++p) wsum[p] = 0.0;

    const int64_t nstage = (nrow + kStage - 1) / kStage;
    for (int64_t st = part; st < nstage; st += nparts) {
        __syncthreads();  // the previous stage has been consumed
        for (int r = threadIdx.x; r < kStage; r += kThreads) {
            // staged row r is row st * kStage + r; rows past nrow are zeros
            const int64_t row = st * kStage + r;
            const bool in = row < nrow;
            double a[3] = {0.0, 0.0, 0.0};
            if (in) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    a[q] = kMetres ? uvw[row * 3 + q] * s : uvw[(row * nchan + chan) * 3 + q];
            }
            s_a[r * 4 + 0] = a[0];
            s_a[r * 4 + 1] = a[1];
            s_a[r * 4 + 2] = a[2];
            s_a[r * 4 + 3] = 0.0;
#pragma unroll
            for (int p = 0; p < NPOL; ++p) {
                VT x;
                x.x = x.y = (FT)0;
                if (in) {
                    const int64_t i = (row * nchan + chan) * NPOL + p;
                    const double wk = weight[i] * keep_of(flags, fbytes, i);
                    const VT v = vis[i];
                    x.x = (FT)wk * v.x;
                    x.y = (FT)wk * v.y;
                    wsum[p] += wk;
                }
                s_x[r * NPOL + p] = x;
            }
        }
        __syncthreads();
        if (c0 >= ncomp) continue;  // ncomp == 0: only W is wanted (block-uniform)

        // complex64: fp32 partial sums of this stage only (32 terms per lane),
        // (re, im) pairs so that the multiply-adds are packed (v_pk_fma_f32)
        floatx2 acc[CC][NPOL];
        if constexpr (!kF64) {
#pragma unroll
            for (int cc = 0; cc < CC; ++cc)
#pragma unroll
                for (int p = 0; p < NPOL; ++p) acc[cc][p] = floatx2{0.0f, 0.0f};
        }
#pragma unroll 1
        for (int t = 0; t < TPW; ++t) {
            const int rb = (wave * TPW + t) * 16;
            const double aop = s_a[(rb + r16) * 4 + k];
            VT x[4][NPOL];  // rows rb + k + 4 i: the rows of this lane's product registers
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int p = 0; p < NPOL; ++p) x[i][p] = s_x[(rb + k + 4 * i) * NPOL + p];
#pragma unroll
            for (int g = 0; g < CC; g += G) {
                doublex4 ph[G];
#pragma unroll
                for (int j = 0; j < G; ++j)
                    ph[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                        aop, bop[g + j], doublex4{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    // x * exp(+2 pi i turns) = x * (cs + i sn)
                    if constexpr (kF64) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            double sn, cs;
                            sincospi(2.0 * __builtin_amdgcn_fract(ph[j][i]), &sn, &cs);
#pragma unroll
                            for (int p = 0; p < NPOL; ++p) {
                                sr[g + j][p] = fma(-x[i][p].y, sn, fma(x[i][p].x, cs, sr[g + j][p]));
                                si[g + j][p] = fma(x[i][p].x, sn, fma(x[i][p].y, cs, si[g + j][p]));
                            }
                        }
                    } else {
                        float sn[4], cs[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float tn = (float)__builtin_amdgcn_fract(ph[j][i]);
                            sn[i] = __builtin_amdgcn_sinf(tn);  // sin(2 pi tn)
                            cs[i] = __builtin_amdgcn_cosf(tn);
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int p = 0; p < NPOL; ++p) {
                                const floatx2 xv{x[i][p].x, x[i][p].y}, xw{-x[i][p].y, x[i][p].x};
                                acc[g + j][p] = __builtin_elementwise_fma(xv, floatx2{cs[i], cs[i]}, acc[g + j][p]);
                                acc[g + j][p] = __builtin_elementwise_fma(xw, floatx2{sn[i], sn[i]}, acc[g + j][p]);
                            }
                    }
                }
            }
        }
        if constexpr (!kF64) {
#pragma unroll
            for (int cc = 0; cc < CC; ++cc)
#pragma unroll
                for (int p = 0; p < NPOL; ++p) {
                    sr[cc][p] += (double)acc[cc][p].x;
                    si[cc][p] += (double)acc[cc][p].y;
                }
        }
    }

    __syncthreads();  // the last stage's LDS reads are done; s_fold is free
    if (do_w) {
        // fixed tree over the 256 threads' fp64 sums, per pol
        double *s_w = reinterpret_cast<double *>(s_fold);
#pragma unroll
        for (int p = 0; p < NPOL; ++p) s_w[p * kThreads + threadIdx.x] = wsum[p];
        __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
#pragma unroll
                for (int p = 0; p < NPOL; ++p)
                    s_w[p * kThreads + threadIdx.x] += s_w[p * kThreads + threadIdx.x + o];
            }
            __syncthreads();
        }
        if (threadIdx.x < NPOL)
            part_w[((int64_t)part * nchan + chan) * NPOL + threadIdx.x] = s_w[threadIdx.x * kThreads];
        __syncthreads();
    }
    if (c0 >= ncomp) return;

    // the 4 lane groups of a wave hold 4 row subsets of the same components
#pragma unroll
    for (int cc = 0; cc < CC; ++cc)
#pragma unroll
        for (int p = 0; p < NPOL; ++p) {
            sr[cc][p] += __shfl_xor(sr[cc][p], 16, 64);
            si[cc][p] += __shfl_xor(si[cc][p], 16, 64);
            sr[cc][p] += __shfl_xor(sr[cc][p], 32, 64);
            si[cc][p] += __shfl_xor(si[cc][p], 32, 64);
        }
    if (k == 0) {
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
#pragma unroll
            for (int p = 0; p < NPOL; ++p)
                s_fold[(wave * kChunk + 16 * cc + r16) * NPOL + p] = make_double2(sr[cc][p], si[cc][p]);
    }
    __syncthreads();
    // waves in order 0..3; scratch is padded to whole chunks, so every
    // element of the chunk is written and none is out of bounds
    for (int e = threadIdx.x; e < kChunk * NPOL; e += kThreads) {
        double2 v = s_fold[e];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            v.x += s_fold[w * kChunk * NPOL + e].x;
            v.y += s_fold[w * kChunk * NPOL + e].y;
        }
        part_s[(((int64_t)part * nchan + chan) * ncomp_pad + c0) * NPOL + e] = v;
    }
}

// S[c, chan, pol] and W[chan, pol]: the partitions' partial sums in index order
__global__ __launch_bounds__(kThreads) void k_idft_reduce(
    int ncomp, int nchan, int npol, int nparts, int ncomp_pad, const double2 *__restrict__ part_s,
    const double *__restrict__ part_w, double2 *__restrict__ flux_sum, double *__restrict__ sumwt) {
    const int64_t ns = (int64_t)ncomp * nchan * npol;
    const int64_t nw = sumwt ? (int64_t)nchan * npol : 0;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < ns) {
        const int p = (int)(i % npol);
        const int chan = (int)((i / npol) % nchan);
        const int64_t c = i / ((int64_t)npol * nchan);
        double2 v = make_double2(0.0, 0.0);
        for (int q = 0; q < nparts; ++q) {
            const double2 t = part_s[(((int64_t)q * nchan + chan) * ncomp_pad + c) * npol + p];
            v.x += t.x;
            v.y += t.y;
        }
        flux_sum[i] = v;
    } else if (i < ns + nw) {
        const int64_t j = i - ns;
        double v = 0.0;
        for (int q = 0; q < nparts; ++q) v += part_w[(int64_t)q * nw + j];
        sumwt[j] = v;
    }
}

template <class VT, bool kMetres, int NPOL>
static void launch_mfma(int ncomp, const double *dc, int64_t nrow, int nchan, const double *uvw,
                        const double *freq, const void *vis, const double *weight,
                        const void *flags, int fbytes, double2 *flux_sum, double *sumwt,
                        hipStream_t st) {
    constexpr int CC = 8 / NPOL;
    constexpr int kChunk = CC * 16;
    constexpr int kStage = 4 * tiles_per_wave<VT>() * 16;
    // ncomp == 0 still runs chunk 0, for W alone
    const int64_t nchunks = std::max<int64_t>(1, ((int64_t)ncomp + kChunk - 1) / kChunk);
    const int64_t ncomp_pad = nchunks * kChunk;
    const int64_t nstage = (nrow + kStage - 1) / kStage;
    // row partitions: enough for about kTargetWgs workgroups, never more than
    // there are stages, capped: scratch is nparts * nchan * ncomp_pad * NPOL
    // * 16 B <= (kTargetWgs + nchunks * nchan) * 128 * 16 B, whatever nrow is
    int64_t nparts = (kTargetWgs + nchunks * nchan - 1) / (nchunks * nchan);
    nparts = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nparts, nstage), kMaxParts));
    if (nparts > 8) nparts &= ~(int64_t)7;  // the chunks of one partition on one XCD
    SDP_REQUIRE(nchan <= 65535 && nchunks <= 65535, "too many channels or components for one IDFT call");
    double2 *part_s = scratch<double2>("idft_part_s", (size_t)(nparts * nchan * ncomp_pad * NPOL));
    double *part_w = sumwt ? scratch<double>("idft_part_w", (size_t)(nparts * nchan * NPOL)) : nullptr;
    k_idft_mfma<NPOL, VT, kMetres, CC>
        <<<dim3((unsigned)nparts, (unsigned)nchunks, (unsigned)nchan), kThreads, 0, st>>>(
            ncomp, dc, nrow, nchan, uvw, freq, static_cast<const VT *>(vis), weight, flags, fbytes,
            (int)nparts, (int)ncomp_pad, part_s, part_w);
    SDP_HIP_CHECK(hipGetLastError());
    const int64_t nout = (int64_t)ncomp * nchan * NPOL + (sumwt ? (int64_t)nchan * NPOL : 0);
    if (nout > 0) {
        SDP_REQUIRE((nout + kThreads - 1) / kThreads < 2147483647, "IDFT output too large");
        k_idft_reduce<<<grid1d(nout, kThreads), kThreads, 0, st>>>(
            ncomp, nchan, NPOL, (int)nparts, (int)ncomp_pad, part_s, part_w, flux_sum, sumwt);
        SDP_HIP_CHECK(hipGetLastError());
    }
}

template <class VT, bool kMetres>
static void launch(int npol, int ncomp, const double *dc, int64_t nrow, int nchan,
                   const double *uvw, const double *freq, const void *vis, const double *weight,
                   const void *flags, int fbytes, double2 *flux_sum, double *sumwt, hipStream_t st) {
    switch (npol) {
        case 1: launch_mfma<VT, kMetres, 1>(ncomp, dc, nrow, nchan, uvw, freq, vis, weight, flags, fbytes, flux_sum, sumwt, st); break;
        case 2: launch_mfma<VT, kMetres, 2>(ncomp, dc, nrow, nchan, uvw, freq, vis, weight, flags, fbytes, flux_sum, sumwt, st); break;
        case 4: launch_mfma<VT, kMetres, 4>(ncomp, dc, nrow, nchan, uvw, freq, vis, weight, flags, fbytes, flux_sum, sumwt, st); break;
        default: throw Error(SDP_HIP_ERR_INVALID_ARG, "npol must be 1, 2 or 4");
    }
}

static void run(bool metres, int ncomp, const double *dc, int npol, int64_t nrow, int nchan,
                const double *uvw, const double *freq, const void *vis, int vis_dtype,
                const double *weight, const void *flags, int flag_bytes, void *flux_sum,
                double *sumwt, hipStream_t st) {
    SDP_REQUIRE(ncomp >= 0 && nrow >= 0 && nchan > 0, "bad sizes");
    SDP_REQUIRE(npol == 1 || npol == 2 || npol == 4, "npol must be 1, 2 or 4");
    SDP_REQUIRE(vis_dtype == SDP_HIP_C64 || vis_dtype == SDP_HIP_C128,
                "vis must be complex64 or complex128");
    SDP_REQUIRE(!flags || flag_bytes == 1 || flag_bytes == 4 || flag_bytes == 8,
                "flag_bytes must be 1, 4 or 8");
    SDP_REQUIRE((ncomp == 0 || (dc && flux_sum)) && (nrow == 0 || (uvw && vis && weight)),
                "null pointer argument");
    SDP_REQUIRE(!metres || freq != nullptr, "freq required with uvw in metres");
    const int fbytes = flags ? flag_bytes : 0;
    double2 *out = static_cast<double2 *>(flux_sum);
    if (nrow == 0) {
        // empty sums: exact zeros
        if (ncomp > 0)
            SDP_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(double2) * (size_t)ncomp * nchan * npol, st));
        if (sumwt) SDP_HIP_CHECK(hipMemsetAsync(sumwt, 0, sizeof(double) * (size_t)nchan * npol, st));
        return;
    }
    if (ncomp == 0 && !sumwt) return;
    if (vis_dtype == SDP_HIP_C128) {
        if (metres)
            launch<double2, true>(npol, ncomp, dc, nrow, nchan, uvw, freq, vis, weight, flags, fbytes, out, sumwt, st);
        else
            launch<double2, false>(npol, ncomp, dc, nrow, nchan, uvw, freq, vis, weight, flags, fbytes, out, sumwt, st);
    } else {
        if (metres)
            launch<float2, true>(npol, ncomp, dc, nrow, nchan, uvw, freq, vis, weight, flags, fbytes, out, sumwt, st);
        else
            launch<float2, false>(npol, ncomp, dc, nrow, nchan, uvw, freq, vis, weight, flags, fbytes, out, sumwt, st);
    }
}

}  // namespace idft
}  // namespace sdp

extern "C" {

int sdp_hip_idft_point_v00(int ncomp, const double *direction_cosines, int npol, int64_t nrow,
                           int nchan, const double *uvw_lambda, const void *vis, int vis_dtype,
                           const double *weight, const void *flags, int flag_bytes,
                           void *flux_sum, double *sumwt, void *stream, char *errbuf,
                           size_t errbuf_len) {
    return sdp::guarded(errbuf, errbuf_len, [&] {
        sdp::idft::run(false, ncomp, direction_cosines, npol, nrow, nchan, uvw_lambda, nullptr, vis,
                       vis_dtype, weight, flags, flag_bytes, flux_sum, sumwt,
                       sdp::as_stream(stream));
    });
}

int sdp_hip_idft_point_metres(int ncomp, const double *direction_cosines, int npol, int64_t nrow,
                              int nchan, const double *uvw, const double *freq, const void *vis,
                              int vis_dtype, const double *weight, const void *flags,
                              int flag_bytes, void *flux_sum, double *sumwt, void *stream,
                              char *errbuf, size_t errbuf_len) {
    return sdp::guarded(errbuf, errbuf_len, [&] {
        sdp::idft::run(true, ncomp, direction_cosines, npol, nrow, nchan, uvw, freq, vis, vis_dtype,
                       weight, flags, flag_bytes, flux_sum, sumwt, sdp::as_stream(stream));
    });
}

}  // extern "C"
