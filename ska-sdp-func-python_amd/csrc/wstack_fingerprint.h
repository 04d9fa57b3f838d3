// w-stacking NUFFT: content fingerprint of the arrays the bucketing layout
// depends on (uvw rows, frequencies).  Order-independent over the elements --
// a wrapping 64-bit sum per word, so the blocks of k_bounds can add their
// partial sums in any order -- but not blind to the order of the content:
// every term mixes the element's index with its bit patterns, so swapping two
// rows or moving a value to another row changes the sums.  Two independent
// 64-bit words per array (128 bits).  Host and device compile the same code
// (the host side: sdp_hip_wstack_fingerprint, the unit tests).
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SDP_FP_HD __host__ __device__
#else
#define SDP_FP_HD
#endif

namespace sdp {
namespace wstack {

// splitmix64's finaliser: a bijection of 64-bit words with full avalanche
SDP_FP_HD inline uint64_t fp_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

SDP_FP_HD inline uint64_t fp_bits(double v) {
    uint64_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = (uint64_t)__double_as_longlong(v);
#else
    std::memcpy(&b, &v, sizeof b);
#endif
    return b;
}

// the two words of one element: `idx` its index (row or channel), `n` values
// (3 for a uvw row, 1 for a frequency); `salt` separates the arrays
SDP_FP_HD inline void fp_term(uint64_t salt, uint64_t idx, const double *v, int n, uint64_t &a,
                              uint64_t &b) {
    uint64_t h = fp_mix(idx + salt);
    for (int k = 0; k < n; ++k)
        h = fp_mix((h ^ fp_bits(v[k])) + 0x9e3779b97f4a7c15ull * (uint64_t)(k + 1));
    a = fp_mix(h);
    b = fp_mix(h ^ 0xd6e8feb86659fd93ull);
}

constexpr uint64_t kFpSaltUvw = 0x243f6a8885a308d3ull;
constexpr uint64_t kFpSaltFreq = 0x13198a2e03707344ull;

// fp[0..1] += the words of uvw row `row`
SDP_FP_HD inline void fp_add_row(uint64_t row, double u, double v, double w, uint64_t &a,
                                 uint64_t &b) {
    const double x[3] = {u, v, w};
    uint64_t ta, tb;
    fp_term(kFpSaltUvw, row, x, 3, ta, tb);
    a += ta;
    b += tb;
}

// fp[0..1] += the words of channel `chan`'s frequency
SDP_FP_HD inline void fp_add_freq(uint64_t chan, double f, uint64_t &a, uint64_t &b) {
    uint64_t ta, tb;
    fp_term(kFpSaltFreq, chan, &f, 1, ta, tb);
    a += ta;
    b += tb;
}

// host reference: out = {uvw a, uvw b, freq a, freq b}
inline void fingerprint_host(const double *uvw, int64_t rs, int64_t nrow, const double *freq,
                             int nchan, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    for (int64_t r = 0; r < nrow; ++r)
        fp_add_row((uint64_t)r, uvw[r * rs], uvw[r * rs + 1], uvw[r * rs + 2], out[0], out[1]);
    for (int c = 0; c < nchan; ++c) fp_add_freq((uint64_t)c, freq[c], out[2], out[3]);
}

}  // namespace wstack
}  // namespace sdp
