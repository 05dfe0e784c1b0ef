// The LDS-resident FFT shared by the STFT kernels (stft.hip: magnitudes and the
// audio distance; stft_loss.hip: the differentiable spectral losses).
//
// Complex fp32, radix-4 Stockham stages (plus one radix-2 stage when log2 n is
// odd) run in place: every thread reads its butterflies' inputs into registers,
// the workgroup meets at a barrier, and the outputs go back to the same arrays
// in the autosort order.  Real and imaginary parts live in separate arrays, so a
// stage's reads are unit-stride.  One workgroup (256 threads) transforms kConc =
// max(1, 1024 / n) frames at once -- one radix-4 butterfly per thread for n <=
// 1024, 2 and 4 for n = 2048 and 4096.
#pragma once

#include "common.h"

namespace rave {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMinN = 64, kMaxN = 4096;

constexpr int ilog2(int n) { return n <= 1 ? 0 : 1 + ilog2(n >> 1); }

template <int N>
struct Geo {
    static constexpr int kConc = N >= 1024 ? 1 : 1024 / N;        // frames transformed at once
    static constexpr int kPasses = N <= 1024 ? 4 : 2;
    static constexpr int kTile = kConc * kPasses;                 // transforms per workgroup
    static constexpr int kBfly = kConc * (N / 4) / kThreads;      // radix-4 butterflies per thread
    static constexpr int kLog = ilog2(N);
    static_assert(kConc * (N / 4) % kThreads == 0 && kBfly >= 1, "butterflies must fill the workgroup");
};

// host mirrors of Geo<n> (n validated)
inline int conc_of(int n) { return n >= 1024 ? 1 : 1024 / n; }
inline int tile_of(int n) { return conc_of(n) * (n <= 1024 ? 4 : 2); }
inline size_t lds_bytes_of(int n) { return (size_t)2 * conc_of(n) * n * sizeof(float); }

inline bool scale_supported(int n) { return n >= kMinN && n <= kMaxN && (n & (n - 1)) == 0; }

// In-place FFT of kConc frames: re / im hold frame slot c at [c*N, (c+1)*N).
// The caller has put a barrier after filling them; the result (natural order)
// is visible to every thread on return.  tw[k] = exp(-2 pi i k / N).
template <int N>
__device__ __forceinline__ void fft_lds(float* re, float* im, const float2* __restrict__ tw) {
    using G = Geo<N>;
    constexpr int Q = N / 4;
#pragma unroll
    for (int st = 0; st < G::kLog / 2; ++st) {
        const int s = 1 << (2 * st);                              // stride of this stage
        float ar[G::kBfly][4], ai[G::kBfly][4];
#pragma unroll
        for (int u = 0; u < G::kBfly; ++u) {
            const int b = threadIdx.x + u * kThreads;
            const int base = (b / Q) * N + (b % Q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ar[u][k] = re[base + k * Q];
                ai[u][k] = im[base + k * Q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < G::kBfly; ++u) {
            const int b = threadIdx.x + u * kThreads;
            const int j = b % Q;
            const int q = j & (s - 1);
            const int e = j - q;                                  // p * s: the twiddle exponent
            const int o = (b / Q) * N + 4 * e + q;                // q + s * 4p
            const float2 w1 = tw[e], w2 = tw[2 * e], w3 = tw[3 * e];
            const float apcr = ar[u][0] + ar[u][2], apci = ai[u][0] + ai[u][2];
            const float amcr = ar[u][0] - ar[u][2], amci = ai[u][0] - ai[u][2];
            const float bpdr = ar[u][1] + ar[u][3], bpdi = ai[u][1] + ai[u][3];
            const float jr = -(ai[u][1] - ai[u][3]), ji = ar[u][1] - ar[u][3];   // j (b - d)
            re[o] = apcr + bpdr;
            im[o] = apci + bpdi;
            const float t1r = amcr - jr, t1i = amci - ji;
            re[o + s] = t1r * w1.x - t1i * w1.y;
            im[o + s] = t1r * w1.y + t1i * w1.x;
            const float t2r = apcr - bpdr, t2i = apci - bpdi;
            re[o + 2 * s] = t2r * w2.x - t2i * w2.y;
            im[o + 2 * s] = t2r * w2.y + t2i * w2.x;
            const float t3r = amcr + jr, t3i = amci + ji;
            re[o + 3 * s] = t3r * w3.x - t3i * w3.y;
            im[o + 3 * s] = t3r * w3.y + t3i * w3.x;
        }
        __syncthreads();
    }
    if (G::kLog & 1) {       // last stage, sub-length 2: each thread rewrites the two elements it read
        constexpr int H = N / 2;
#pragma unroll
        for (int u = 0; u < 2 * G::kBfly; ++u) {
            const int b = threadIdx.x + u * kThreads;
            const int i0 = (b / H) * N + (b % H);
            const float xr = re[i0], xi = im[i0], yr = re[i0 + H], yi = im[i0 + H];
            re[i0] = xr + yr;
            im[i0] = xi + yi;
            re[i0 + H] = xr - yr;
            im[i0 + H] = xi - yi;
        }
        __syncthreads();
    }
}

// center=True, pad_mode="reflect": sample index of padded position i - N/2.
// One reflection is enough because N/2 < t_len (checked on the host).
__device__ __forceinline__ int reflect(int i, int t_len) {
    if (i < 0) i = -i;
    if (i >= t_len) i = 2 * (t_len - 1) - i;
    return i;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace
}  // namespace rave
