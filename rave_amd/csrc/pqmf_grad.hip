// Adjoints of the PQMF filterbank kernels (gfx950): the backward passes of
// rave_pqmf_synthesis and rave_pqmf_analysis (pqmf.hip), exact fp32 only.
//
// Both forward maps are linear (mode 0 of the synthesis in x; modes 1 / 2 put
// GeneratorV2's epilogue in front), and both adjoints are 33-tap FIR GEMMs of
// the forward synthesis' shape: 16 output rows, K = channels x 33, one column
// per frame, on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain).
//
//   synthesis  gv[b, c, f] = 16 rh(c, frame0 + f) sum_{k, i} hki[15 - i, c, k] gy[b, 16 (f - k + pad_left) + i]
//              rows c, K ordered (k, i), B = the de-interleaved cotangent
//   analysis   gx[b, 16 u + i] = sum_{d, k} hkf[k, 16 d + i] rh(k, t) gy[b, k, t],  t = u + pad_left / 16 - d
//              rows i (the 16 output phases), K ordered (d, k), d < 33, k < n_out_bands
//
// Frames t outside the cotangent read as zero.  Every output element is one
// gather, written once by a plain vector-memory store: no atomics, no
// workspace, and two calls agree bit for bit.
#include "common.h"

namespace rave {

typedef float pg_f32x4 __attribute__((ext_vector_type(4)));

// pqmf.hip's geometry: a wave owns two blocks of 16 columns, a workgroup 128
// columns; window rows at a stride of 25 mod 32, filter rows at K + 9.
constexpr int kPgWaves = 4;
constexpr int kPgBlk = 2;
constexpr int kPgCols = kPgWaves * kPgBlk * 16;              // output columns per workgroup (128)
constexpr int kPgTaps = 33;                                  // frame taps of both adjoints
constexpr int kPgXW = kPgCols + kPgTaps - 1;                 // window frames (160)
constexpr int kPgXR = kPgXW + ((25 - kPgXW % 32) + 32) % 32; // row stride = 25 mod 32
constexpr int kPgNT = 64 * kPgWaves;

// acc[q][r] = sum_K hs[row 4 kk + r][K] ws[K][column], K = tap * KB + channel in
// ascending order: step s covers channels 4 (s % (KB / 4)) .. + 3 of tap
// s / (KB / 4); window column w holds frame (first column) - 32 + w, so tap d of
// column c reads w = c + 32 - d.  Every LDS offset is a compile-time immediate.
template <int KB, int HR>
__device__ __forceinline__ void pg_gemm(const float* hs, const float* ws, pg_f32x4 (&acc)[kPgBlk]) {
    constexpr int kg = KB / 4, ksteps = kPgTaps * kg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kk = lane >> 4, col = lane & 15;
    const int fb = wave * kPgBlk * 16;
#pragma unroll
    for (int q = 0; q < kPgBlk; ++q) acc[q] = pg_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ha = hs + col * HR + kk;
    const float* xl = ws + kk * kPgXR + fb + col;
#pragma unroll
    for (int s = 0; s < ksteps; ++s) {
        const float av = ha[4 * s];
#pragma unroll
        for (int q = 0; q < kPgBlk; ++q)
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                av, xl[(4 * (s % kg)) * kPgXR + (kPgTaps - 1 - s / kg) + q * 16], acc[q], 0, 0, 0);
    }
}

// The epilogue's derivative at one element, from the saved forward inputs:
// u = fma(x_w, sg, n) with sg = sigmoid(x_a) (mode 1) or 1 (mode 2), t = tanh(u),
// gn = gv fma(-t, t, 1), gx_w = gn sg, gx_a = (gn x_w) (sg (1 - sg)).
struct pg_grads {
    float gn, gw, ga;
};
__device__ __forceinline__ pg_grads pg_epilogue(int mode, float gv, float xw, float xa, float n) {
#pragma clang fp contract(off)
    float sg = 1.0f;
    if (mode == 1) sg = 1.0f / (1.0f + expf(-xa));
    const float t = tanhf(fmaf(xw, sg, n));
    pg_grads g;
    g.gn = gv * fmaf(-t, t, 1.0f);
    g.gw = g.gn * sg;
    g.ga = (g.gn * xw) * (sg * (1.0f - sg));
    return g;
}

// ---------------------------------------------------------------- synthesis backward
constexpr int kPgSynK = 16 * kPgTaps;                        // 528
constexpr int kPgSynHR = kPgSynK + 9;                        // 537 (25 mod 32)
__global__ __launch_bounds__(kPgNT) void pqmf_synthesis_backward_kernel(rave_pqmf_synthesis_backward_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* hs = smem;                        // [16 rows c][kPgSynHR], K = k * 16 + i
    float* gs = smem + 16 * kPgSynHR;        // [16 phases i][kPgXR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lg_ = __builtin_amdgcn_readfirstlane(
        xcd_major(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y));
    const int b = lg_ / gridDim.x;
    const int n0 = (lg_ - b * gridDim.x) * kPgCols;
    // every load of a thread is issued before its first LDS store
    {
        constexpr int HT = (16 * kPgSynHR + kPgNT - 1) / kPgNT;
        float hv[HT];
#pragma unroll
        for (int it = 0; it < HT; ++it) {
            const int i = tid + it * kPgNT;
            const int c = i / kPgSynHR;
            const int k = i - c * kPgSynHR;
            const int kc = min(k, kPgSynK - 1);
            const float v = a.hki[(int64_t)(15 - (kc & 15)) * kPgSynK + min(c, 15) * kPgTaps + (kc >> 4)];
            hv[it] = (i < 16 * kPgSynHR && k < kPgSynK) ? v : 0.f;
        }
#pragma unroll
        for (int it = 0; it < HT; ++it) {
            const int i = tid + it * kPgNT;
            if (i < 16 * kPgSynHR) hs[i] = hv[it];
        }
    }
    const float* gyb = a.gy + (int64_t)b * a.gy_sb;
    const int w0 = n0 + a.pad_left - (kPgTaps - 1);          // frame of window column 0
    {
        // window element (i, w) = gy[16 (w0 + w) + i]: consecutive threads read consecutive samples
        constexpr int XT = 16 * kPgXW / kPgNT;
        static_assert(XT * kPgNT == 16 * kPgXW, "window loop");
        float gv[XT];
#pragma unroll
        for (int it = 0; it < XT; ++it) {
            const int i = tid + it * kPgNT;
            const int t = w0 + (i >> 4);
            const float v = gyb[(int64_t)min(max(t, 0), a.t_in - 1) * 16 + (i & 15)];
            gv[it] = (t >= 0 && t < a.t_in) ? v : 0.f;
        }
#pragma unroll
        for (int it = 0; it < XT; ++it) {
            const int i = tid + it * kPgNT;
            gs[(i & 15) * kPgXR + (i >> 4)] = gv[it];
        }
    }
    __syncthreads();
    const int kk = lane >> 4, col = lane & 15;
    const int fb = wave * kPgBlk * 16;
    const int x_len = a.x_len > 0 ? a.x_len : a.t_in;
    // the saved inputs of this lane's outputs (row c = 4 kk + r, column f), loaded ahead of the GEMM
    float xw[kPgBlk][4] = {}, xa[kPgBlk][4] = {}, nz[kPgBlk][4] = {};
    if (a.mode != 0) {                                        // uniform branch
        const float* xb = a.x + (int64_t)b * a.x_sb;
        const float* nzb = a.noise ? a.noise + (int64_t)b * a.n_sb : nullptr;
#pragma unroll
        for (int q = 0; q < kPgBlk; ++q) {
            const int f = min(n0 + fb + q * 16 + col, x_len - 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 4 * kk + r;
                xw[q][r] = xb[(int64_t)c * a.x_sc + f];
                xa[q][r] = xb[(int64_t)(a.mode == 1 ? c + 16 : c) * a.x_sc + f];
                nz[q][r] = nzb ? nzb[(int64_t)c * a.n_sc + f] : 0.f;
            }
        }
    }
    pg_f32x4 acc[kPgBlk];
    pg_gemm<16, kPgSynHR>(hs, gs, acc);
    float* gxb = a.gx + (int64_t)b * a.gx_sb;
    float* gnb = a.gnoise ? a.gnoise + (int64_t)b * a.gn_sb : nullptr;
#pragma unroll
    for (int q = 0; q < kPgBlk; ++q) {
        const int f = n0 + fb + q * 16 + col;
        if (f >= x_len) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 4 * kk + r;
            float gv = 16.f * acc[q][r];
            if ((c & 1) && !((a.frame0 + f) & 1)) gv = -gv;   // reverse_half
            if (a.mode == 0) {
                gxb[(int64_t)c * a.gx_sc + f] = gv;
                continue;
            }
            const pg_grads g = pg_epilogue(a.mode, gv, xw[q][r], xa[q][r], nz[q][r]);
            gxb[(int64_t)c * a.gx_sc + f] = g.gw;
            if (a.mode == 1) gxb[(int64_t)(c + 16) * a.gx_sc + f] = g.ga;
            if (gnb) gnb[(int64_t)c * a.gn_sc + f] = g.gn;
        }
    }
}

// ---------------------------------------------------------------- analysis backward
// KB = n_out_bands rounded up to the MFMA's K of 4 (rows >= NBO of the window
// and of the filter image are zero: they add exact zeros to the chain).
template <int NBO>
__global__ __launch_bounds__(kPgNT) void pqmf_analysis_backward_kernel(rave_pqmf_analysis_backward_args a) {
    constexpr int KB = (NBO + 3) / 4 * 4, K = kPgTaps * KB, HR = K + 9;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* hs = smem;                        // [16 phases i][HR], K = d * KB + k
    float* gs = smem + 16 * HR;              // [KB bands][kPgXR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lg_ = __builtin_amdgcn_readfirstlane(
        xcd_major(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y));
    const int b = lg_ / gridDim.x;
    const int u0 = (lg_ - b * gridDim.x) * kPgCols;
    {
        constexpr int HT = (16 * HR + kPgNT - 1) / kPgNT;
        float hv[HT];
#pragma unroll
        for (int it = 0; it < HT; ++it) {
            const int lin = tid + it * kPgNT;
            const int i = lin / HR;
            const int kq = lin - i * HR;
            const int kc = min(kq, K - 1);
            const int d = kc / KB, k = kc % KB;
            const int j = 16 * d + min(i, 15);                // tap index
            const float v = a.hkf[(int64_t)min(k, NBO - 1) * a.taps + min(j, a.taps - 1)];
            hv[it] = (lin < 16 * HR && kq < K && k < NBO && j < a.taps) ? v : 0.f;
        }
#pragma unroll
        for (int it = 0; it < HT; ++it) {
            const int lin = tid + it * kPgNT;
            if (lin < 16 * HR) hs[lin] = hv[it];
        }
    }
    const float* gyb = a.gy + (int64_t)b * a.gy_sb;
    const int w0 = u0 + a.pad_left / 16 - (kPgTaps - 1);     // frame of window column 0
    {
        constexpr int XT = KB * kPgXW / kPgNT;
        static_assert(XT * kPgNT == KB * kPgXW, "window loop");
        float gv[XT];
#pragma unroll
        for (int it = 0; it < XT; ++it) {
            const int lin = tid + it * kPgNT;
            const int k = lin / kPgXW;
            const int t = w0 + lin - k * kPgXW;
            float v = gyb[(int64_t)min(k, NBO - 1) * a.gy_sc + min(max(t, 0), a.t_out - 1)];
            if ((k & 1) && !(t & 1)) v = -v;                  // reverse_half
            gv[it] = (k < NBO && t >= 0 && t < a.t_out) ? v : 0.f;
        }
#pragma unroll
        for (int it = 0; it < XT; ++it) {
            const int lin = tid + it * kPgNT;
            const int k = lin / kPgXW;
            gs[k * kPgXR + lin - k * kPgXW] = gv[it];
        }
    }
    __syncthreads();
    pg_f32x4 acc[kPgBlk];
    pg_gemm<KB, HR>(hs, gs, acc);
    // D: row = phase 4 kk + r, column = frame u: four consecutive samples per lane
    const int kk = lane >> 4, col = lane & 15;
    const int fb = wave * kPgBlk * 16;
    float* gxb = a.gx + (int64_t)b * a.gx_sb;
    const bool vec = reinterpret_cast<uintptr_t>(gxb) % 16 == 0;
#pragma unroll
    for (int q = 0; q < kPgBlk; ++q) {
        const int64_t s = (int64_t)(u0 + fb + q * 16 + col) * 16 + 4 * kk;
        if (vec && s + 3 < a.t_in) {
            *reinterpret_cast<pg_f32x4*>(gxb + s) = acc[q];
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (s + r < a.t_in) gxb[s + r] = acc[q][r];
        }
    }
}

template <int NBO>
static void launch_analysis_backward(const rave_pqmf_analysis_backward_args& a, void* stream) {
    constexpr int KB = (NBO + 3) / 4 * 4, HR = kPgTaps * KB + 9;
    const size_t lds = (size_t)(16 * HR + KB * kPgXR) * sizeof(float);
    dim3 grid(ceil_div(ceil_div(a.t_in, 16), kPgCols), a.batch);
    launch(pqmf_analysis_backward_kernel<NBO>, grid, dim3(kPgNT), lds, as_stream(stream), a);
}

}  // namespace rave

using namespace rave;

extern "C" int rave_pqmf_synthesis_backward(const rave_pqmf_synthesis_backward_args* p, void* stream) {
    RAVE_CHECK_ARG(p && p->gy && p->gx && p->hki, "pqmf_synthesis_backward: null pointer");
    const rave_pqmf_synthesis_backward_args& a = *p;
    RAVE_CHECK_ARG(a.n_band == 16, "pqmf_synthesis_backward: kernel is built for 16 bands");
    RAVE_CHECK_ARG(a.taps > 0 && a.taps <= 64, "pqmf_synthesis_backward: bad taps");
    RAVE_CHECK_ARG(a.batch > 0 && a.t_in > 0 && a.x_len >= 0, "pqmf_synthesis_backward: empty shape");
    RAVE_CHECK_ARG(a.mode >= 0 && a.mode <= 2, "pqmf_synthesis_backward: mode must be 0, 1 or 2");
    RAVE_CHECK_ARG(a.mode == 0 || a.x, "pqmf_synthesis_backward: modes 1 and 2 need the saved input x");
    if (a.taps != kPgTaps) {
        set_error("pqmf_synthesis_backward: kernel is built for the 33-tap RAVE synthesis filter");
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(a.precision == RAVE_PREC_F32, "pqmf_synthesis_backward: precision must be RAVE_PREC_F32");
    const int x_len = a.x_len > 0 ? a.x_len : a.t_in;
    const size_t lds = (size_t)(16 * kPgSynHR + 16 * kPgXR) * sizeof(float);
    dim3 grid(ceil_div(x_len, kPgCols), a.batch);
    launch(pqmf_synthesis_backward_kernel, grid, dim3(kPgNT), lds, as_stream(stream), a);
    return launch_status("pqmf_synthesis_backward_kernel");
}

extern "C" int rave_pqmf_analysis_backward(const rave_pqmf_analysis_backward_args* p, void* stream) {
    RAVE_CHECK_ARG(p && p->gy && p->gx && p->hkf, "pqmf_analysis_backward: null pointer");
    const rave_pqmf_analysis_backward_args& a = *p;
    RAVE_CHECK_ARG(a.n_band == 16, "pqmf_analysis_backward: kernel is built for 16 bands");
    RAVE_CHECK_ARG(a.n_out_bands == 6 || a.n_out_bands == 16,
                   "pqmf_analysis_backward: n_out_bands must be 6 (RAVE.encode) or 16");
    RAVE_CHECK_ARG(a.taps > 0 && a.taps <= 1024, "pqmf_analysis_backward: bad taps");
    RAVE_CHECK_ARG(a.batch > 0 && a.t_in > 0 && a.t_out > 0, "pqmf_analysis_backward: empty shape");
    RAVE_CHECK_ARG(a.pad_left >= 0 && a.pad_left % 16 == 0,
                   "pqmf_analysis_backward: pad_left must be a non-negative multiple of 16");
    if ((a.taps + 3) / 4 != 129) {
        set_error("pqmf_analysis_backward: kernel is built for the 513-tap RAVE prototype");
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(a.precision == RAVE_PREC_F32, "pqmf_analysis_backward: precision must be RAVE_PREC_F32");
    if (a.n_out_bands == 6)
        launch_analysis_backward<6>(a, stream);
    else
        launch_analysis_backward<16>(a, stream);
    return launch_status("pqmf_analysis_backward_kernel");
}
