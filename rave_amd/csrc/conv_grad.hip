// Backward of rave_conv1d (gfx950), exact fp32 only: the data gradient, the
// weight / bias gradient and Snake's alpha gradient, of the non-transposed conv
// and of the offline ConvTranspose1d.  The families share the split-K slab
// layout, the slab and alpha reduce kernels and the host side.  The two data kernels keep an epilogue each, word for word the
// same but for the time index (t = u s + p against t = u): the transposed one at
// r = 4 sits on the 256-register limit, where its speed follows any change of its
// text, so folding the two waits for that kernel's staging batch to shrink.
//
// With a = act(x), zero outside [0, t_in), and the forward
//   y[b, m, n] = bias[m] + sum_{ci, j} W[m, ci, j] a[b, ci, n s + j d - pl]  (+ res[b, m, n])
// the kernels here compute
//   ga[b, ci, t] = sum_{j, m} W[m, ci, j] gy[b, m, (t + pl - j d) / s]     gx = ga act'(x)
//   gW[m, ci, j] = sum_{b, n} gy[b, m, n] a[b, ci, n s + j d - pl]          gbias[m] = sum_{b, n} gy[b, m, n]
//   galpha[ci]   = sum_{b, t} ga[b, ci, t] d act / d alpha (x[b, ci, t])
// on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per output element).
//
// data:   rows ci, columns u of one output phase p (t = s u + p), K = (i, m): phase p
//         sees the k / s taps j = j0 + s i, j0 = (p + pl) mod s, at
//         n = u + (p + pl) / s - i d, a stride-1 gather.  The s phases are s
//         sub-problems (grid z = batch x phase): no column is computed and dropped.
// weight: rows m, columns (j, ci) in blocks of 16 ci per tap, K = (b, n); the grid's
//         z splits K into slabs, summed in slab order by a second launch.
// Both operands sit in LDS as [channel][time] rows whose strides make every
// fragment read (ds_read_b32: banks mod 32 per 32-lane half) conflict-free:
// the operand whose 16 lanes walk time needs a row stride of 16 mod 32 (the
// other half's two k rows then land on the other 16 banks); the operand whose
// 16 lanes walk channels needs a row stride of 2 x odd (banks 2 row' + k).
//
// No atomics; nothing in the workspace needs zeroing; every output element is
// written once by a plain vector-memory store; two calls agree bit for bit.
#include "conv_shared.h"

namespace rave {

struct CgArgs {
    const float* x; const float* gy; const float* w; const float* alpha;
    float* gx; float* gw; float* gb; float* galpha;
    float* slabs;                 // weight split-K slabs (S > 1)
    float* apart;                 // alpha partials, (workgroups of the data grid per ci tile) x c_in
    int64_t x_sb, x_sc, gy_sb, gy_sc, gx_sb, gx_sc;
    int c_in, c_out, k, s, d, pl, t_in, t_out, B, act;
    float slope;
    int S, cps, nch, tch;         // weight: K splits, chunks per split, chunks, chunks per batch item
    int P;                        // alpha partial rows
};

// sin(2 z) and sin(z)^2 on sin_squared's reduction and polynomials (common.h):
// z = r + q pi/2, so sin(2 z) = (-1)^q 2 sin r cos r and sin(z)^2 = q odd ? cos(r)^2 : sin(r)^2.
__device__ __forceinline__ void snake_parts(float z, float& sin2, float& ssq) {
    const float q = rintf(z * 0.636619772367581343f);
    float r = fmaf(q, -1.57079637050628662109375f, z);
    r = fmaf(q, 4.371138828673793e-08f, r);
    r = fmaf(q, 1.7151245100058819e-15f, r);
    const float zz = r * r;
    const float s = fmaf(fmaf(fmaf(-1.9515295891e-4f, zz, 8.3321608736e-3f), zz, -1.6666654611e-1f), zz * r, r);
    const float c = fmaf(fmaf(fmaf(2.443315711809948e-5f, zz, -1.388731625493765e-3f), zz,
                              4.166664568298827e-2f),
                         zz * zz, fmaf(-0.5f, zz, 1.0f));
    const bool odd = (static_cast<int>(q) & 1) != 0;
    const float p2 = 2.0f * s * c;
    sin2 = odd ? -p2 : p2;
    ssq = odd ? c * c : s * s;
}

// ---------------------------------------------------------------- what the two families share
// galpha[ci] = the partial rows in row order: one wave per ci, lane l takes rows
// l, l + 64, ... in order, then a fixed butterfly.
__global__ __launch_bounds__(64) void conv1d_grad_alpha_reduce_kernel(CgArgs a) {
    const int ci = blockIdx.x, lane = threadIdx.x;
    float v = 0.f;
    for (int r = lane; r < a.P; r += 64) v += a.apart[(int64_t)r * a.c_in + ci];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) a.galpha[ci] = v;
}

// Split-K of the weight kernels: one slab layout for both families.  A slab is gweight in torch's
// own layout (c_in c_out k floats, whichever channel leads), then c_out bias sums; a kernel stores
// through dst = unsplit ? gweight : slab with one index, and a slab's weights only when gweight is
// asked for.
// Sum the slabs in slab order into gweight and gbias; an output not asked for is not read.
__global__ __launch_bounds__(256) void grad_slab_reduce_kernel(CgArgs a) {
    const int64_t WN = (int64_t)a.c_in * a.c_out * a.k, total = WN + a.c_out;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const bool bias = i >= WN;
        if (bias ? a.gb == nullptr : a.gw == nullptr) continue;
        float v = 0.f;
        for (int s = 0; s < a.S; ++s) v += a.slabs[(int64_t)s * total + i];
        if (bias)
            a.gb[i - WN] = v;
        else
            a.gw[i] = v;
    }
}

// ---------------------------------------------------------------- data gradient
constexpr int kDgCT = 32;          // ci rows per workgroup (two MFMA row blocks)
constexpr int kDgTN = 128;         // columns u per workgroup: 32 per wave (two column blocks)
constexpr int kDgMC = 16;          // output channels m per staged K chunk
constexpr int kDgXR = 176;         // gy window row stride: >= 128 + 2 * 16, 16 mod 32
constexpr int kDgWR = 48;          // weight row stride: >= 32, 16 mod 32
constexpr int kDgMaxNI = 7;        // taps per phase (k / s)
static_assert(kDgXR % 32 == 16 && kDgWR % 32 == 16, "fragment reads: the two k rows of a half on disjoint banks");
static_assert(kDgXR >= kDgTN + 2 * kMaxDil && kDgXR >= kDgTN + kDgMaxNI - 1, "window row");

__global__ __launch_bounds__(256) void conv1d_grad_data_kernel(CgArgs a) {
    __shared__ float gs[kDgMC * kDgXR];                   // [m][window column]
    __shared__ float wsm[kDgMaxNI * kDgMC * kDgWR];       // [i][m][ci]
    __shared__ float red[4 * kDgCT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = lane >> 4, col = lane & 15;
    const int bz = blockIdx.z;
    const int b = bz / a.s, p = bz - b * a.s;
    const int j0 = (p + a.pl) % a.s, q = (p + a.pl) / a.s;
    const int NI = a.k / a.s;
    const int U = p < a.t_in ? (a.t_in - p + a.s - 1) / a.s : 0;   // columns of this phase
    const int u0 = blockIdx.x * kDgTN, ci0 = blockIdx.y * kDgCT;
    const bool want_alpha = a.act == RAVE_ACT_SNAKE && a.apart != nullptr;
    float* aprow = want_alpha ? a.apart + ((int64_t)bz * gridDim.x + blockIdx.x) * a.c_in : nullptr;
    if (u0 >= U) {                                        // uniform: an empty tile of a short phase
        if (want_alpha && tid < kDgCT && ci0 + tid < a.c_in) aprow[ci0 + tid] = 0.f;
        return;
    }
    const int XW = kDgTN + (NI - 1) * a.d;                // window columns
    const int nw0 = u0 + q - (NI - 1) * a.d;              // n of window column 0
    const float* gyb = a.gy + (int64_t)b * a.gy_sb;
    const int wci = tid / NI, wi = tid - wci * NI;        // this thread's (ci, i) of the weight chunk

    f32x4 acc[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int m0 = 0; m0 < a.c_out; m0 += kDgMC) {
        __syncthreads();
        {
            float gv[kDgMC], wv[kDgMC];
            const int n = nw0 + tid;
            const bool nok = tid < XW && n >= 0 && n < a.t_out;
            const bool wok = tid < kDgCT * NI && ci0 + wci < a.c_in;
#pragma unroll
            for (int m = 0; m < kDgMC; ++m) {
                const bool mok = m0 + m < a.c_out;
                gv[m] = (nok && mok) ? gyb[(int64_t)(m0 + m) * a.gy_sc + n] : 0.f;
                wv[m] = (wok && mok) ? a.w[((int64_t)(m0 + m) * a.c_in + ci0 + wci) * a.k + j0 + a.s * wi] : 0.f;
            }
#pragma unroll
            for (int m = 0; m < kDgMC; ++m) {
                if (tid < XW) gs[m * kDgXR + tid] = gv[m];
                if (tid < kDgCT * NI) wsm[(wi * kDgMC + m) * kDgWR + wci] = wv[m];
            }
        }
        __syncthreads();
        for (int i = 0; i < NI; ++i) {
            const float* wa = wsm + (i * kDgMC + kk) * kDgWR + col;
            const float* gb = gs + kk * kDgXR + wave * 32 + col + (NI - 1 - i) * a.d;
#pragma unroll
            for (int ms = 0; ms < kDgMC / 4; ++ms) {
                const float a0 = wa[4 * ms * kDgWR], a1 = wa[4 * ms * kDgWR + 16];
                const float b0 = gb[4 * ms * kDgXR], b1 = gb[4 * ms * kDgXR + 16];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    // D: row ci = 4 kk + r of the row block, column = col of the column block
    const float* xb = a.x ? a.x + (int64_t)b * a.x_sb : nullptr;
    float* gxb = a.gx ? a.gx + (int64_t)b * a.gx_sb : nullptr;
    float asum[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = ci0 + rb * 16 + 4 * kk + r;
            const bool cok = ci < a.c_in;
            float al = 0.f, rr = 0.f;
            if (a.act == RAVE_ACT_SNAKE) {
                al = a.alpha[cok ? ci : 0];
                rr = 1.0f / (al + 1e-9f);
            }
            float sum = 0.f;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const int u = u0 + wave * 32 + cb * 16 + col;
                const int64_t t = (int64_t)u * a.s + p;
                const bool ok = cok && t < a.t_in;
                const float ga = acc[rb][cb][r];
                float g = ga;
                if (a.act != RAVE_ACT_NONE) {
                    const float xv = ok ? xb[(int64_t)ci * a.x_sc + t] : 0.f;
                    if (a.act == RAVE_ACT_LEAKY) {
                        g = xv > 0.f ? ga : ga * a.slope;
                    } else {
                        float sin2, ssq;
                        snake_parts(al * xv, sin2, ssq);
                        g = ga * fmaf(al * rr, sin2, 1.0f);
                        const float da = (xv * sin2) * rr - (ssq * rr) * rr;
                        sum += ok ? ga * da : 0.f;
                    }
                }
                if (ok && gxb) gxb[(int64_t)ci * a.gx_sc + t] = g;
            }
            asum[rb][r] = sum;
        }
    }
    if (want_alpha) {                                     // uniform
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = asum[rb][r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
                if (col == 0) red[wave * kDgCT + rb * 16 + 4 * kk + r] = v;
            }
        __syncthreads();
        if (tid < kDgCT && ci0 + tid < a.c_in)
            aprow[ci0 + tid] = ((red[tid] + red[kDgCT + tid]) + red[2 * kDgCT + tid]) + red[3 * kDgCT + tid];
    }
}

// ---------------------------------------------------------------- weight gradient
constexpr int kWgMT = 64;          // rows m per workgroup: one MFMA row block per wave
constexpr int kWgCT = 16;          // input channels per workgroup: one column block per tap
constexpr int kWgTK = 64;          // output columns n per staged K chunk
constexpr int kWgHR = 66;          // gy row stride: 2 x 33
constexpr int wg_stride(int kt) { return kt == 4 ? 2 : kt == 8 ? 4 : 1; }
// columns of the staged input window at the largest dilation, per phase, and the row stride (2 x odd)
constexpr int wg_xwin(int kt) { return (kWgTK - 1) * wg_stride(kt) + (kt - 1) * (kt == 3 ? kMaxDil : 1) + 1; }
constexpr int wg_pr(int kt) { return ceil_div(wg_xwin(kt), wg_stride(kt)); }
constexpr int wg_xr(int kt) { return (wg_pr(kt) * wg_stride(kt) + 1) / 4 * 4 + 2; }
static_assert(kWgHR % 4 == 2 && kWgHR >= kWgTK, "gy rows: banks 2 row' + k");

template <int KT>
__global__ __launch_bounds__(256) void conv1d_grad_weight_kernel(CgArgs a) {
    constexpr int ST = wg_stride(KT), PR = wg_pr(KT), XR = wg_xr(KT);
    static_assert(XR % 4 == 2 && XR >= PR * ST, "window rows: banks 2 row' + k");
    static_assert(kWgTK - 1 + (KT - 1) / ST < PR || ST == 1, "phase row");
    __shared__ float gys[kWgMT * kWgHR];                  // [m][n]
    __shared__ float xs[kWgCT * XR];                      // [ci][phase][column / s], act applied
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = lane >> 4, col = lane & 15;
    const int m0 = blockIdx.x * kWgMT, ci0 = blockIdx.y * kWgCT, sp = blockIdx.z;
    const int XW = (kWgTK - 1) * ST + (KT - 1) * a.d + 1;
    f32x4 acc[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const int ch_end = min((sp + 1) * a.cps, a.nch);
    for (int ch = sp * a.cps; ch < ch_end; ++ch) {
        const int b = ch / a.tch;
        const int n0 = (ch - b * a.tch) * kWgTK;
        const float* gyb = a.gy + (int64_t)b * a.gy_sb;
        const float* xb = a.x + (int64_t)b * a.x_sb;
        const int tw0 = n0 * ST - a.pl;                   // t of window column 0
        __syncthreads();
        {
            constexpr int GT = kWgMT * kWgTK / 256;
            float gv[GT];
#pragma unroll
            for (int it = 0; it < GT; ++it) {
                const int e = tid + it * 256;
                const int m = m0 + (e >> 6), n = n0 + (e & 63);
                gv[it] = (m < a.c_out && n < a.t_out) ? gyb[(int64_t)m * a.gy_sc + n] : 0.f;
            }
#pragma unroll
            for (int it = 0; it < GT; ++it) {
                const int e = tid + it * 256;
                gys[(e >> 6) * kWgHR + (e & 63)] = gv[it];
            }
        }
        for (int w = tid; w < XW; w += 256) {
            const int t = tw0 + w;
            // a column counts only if a valid output n < t_out reads it through some tap: the
            // columns a stride's right tail or a dilation's gaps leave unread (a NaN there must
            // not meet the zero cotangent of a masked n) stage as zeros.  Bias only: x unread.
            bool used = false;
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                const int r = w - j * (ST == 1 ? a.d : 1);
                if (r >= 0 && r % ST == 0 && r / ST < kWgTK && n0 + r / ST < a.t_out) used = true;
            }
            const bool tok = a.gw != nullptr && used && t >= 0 && t < a.t_in;
            const int dst = (w % ST) * PR + w / ST;
            float xv[kWgCT];
#pragma unroll
            for (int c = 0; c < kWgCT; ++c)
                xv[c] = (tok && ci0 + c < a.c_in) ? xb[(int64_t)(ci0 + c) * a.x_sc + t] : 0.f;
#pragma unroll
            for (int c = 0; c < kWgCT; ++c) {
                float v = xv[c];
                if (a.act != RAVE_ACT_NONE && tok && ci0 + c < a.c_in)
                    v = apply_act(v, a.act, a.slope, a.act == RAVE_ACT_SNAKE ? a.alpha[ci0 + c] : 0.f);
                xs[c * XR + dst] = v;
            }
        }
        __syncthreads();
        const float* ga = gys + (wave * 16 + col) * kWgHR + kk;
        const float* xa = xs + col * XR + kk;
#pragma unroll 4
        for (int st = 0; st < kWgTK / 4; ++st) {
            const float av = ga[4 * st];
            bsum += av;
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                const int off = ST == 1 ? j * a.d : (j % ST) * PR + j / ST;
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xa[off + 4 * st], acc[j], 0, 0, 0);
            }
        }
    }
    // D: row m = 4 kk + r of this wave's row block, column ci = col
    const int64_t WN = (int64_t)a.c_in * a.c_out * KT;    // slab: the weights, then c_out bias sums
    const bool direct = a.S == 1;
    float* dst = direct ? a.gw : a.slabs + (int64_t)sp * (WN + a.c_out);
    const int ci = ci0 + col;
    if (a.gw && ci < a.c_in) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wave * 16 + 4 * kk + r;
            if (m >= a.c_out) continue;
#pragma unroll
            for (int j = 0; j < KT; ++j) dst[((int64_t)m * a.c_in + ci) * KT + j] = acc[j][r];
        }
    }
    // gbias: this lane's A values are row `col`, k = kk: sum the four k lanes
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    const int m = m0 + wave * 16 + lane;
    if (blockIdx.y == 0 && lane < 16 && m < a.c_out) {
        if (!direct)
            dst[WN + m] = bsum;
        else if (a.gb)
            a.gb[m] = bsum;
    }
}

// ---------------------------------------------------------------- transposed conv
// Backward of the offline ConvTranspose1d(c_in, c_out, 2 r, stride r, padding r/2), r = 2 or 4,
// W in torch's layout (c_in, c_out, 2 r), P = r/2:
//   ga[b, ci, u]  = sum_{m, j} W[ci, m, j] gy[b, m, u r + j - P]           gx = ga act'(x)
//   gW[ci, m, j]  = sum_{b, u} a[b, ci, u] gy[b, m, u r + j - P]           gbias[m] = sum_{b, t} gy[b, m, t]
// Both kernels stage their gy window de-interleaved by phase: window column w
// (t = (u0 - 1) r + w) sits at [m][w mod r][w / r], so tap j of column u is phase
// q(j) = (j + r/2) mod r at index (u - u0) + sh(j), sh(j) = (j + r/2) / r in {0, 1, 2}: a
// fragment walks u at stride 1.
//
// data:   rows ci, columns u, K = (m, j) with the four k of an MFMA four taps of one m: the A
//         fragment is then four consecutive floats of W's own row, and the weight chunk is a
//         straight copy of 16 m x 2 r floats per ci row (row stride 2 x odd: banks 2 ci' + k).
//         The B fragment's two k of a 32-lane half are taps j, j + 1 (j even), whose window rows
//         differ by the phase stride (r = 4) or by 1 - the phase stride (r = 2): a phase stride
//         of 16 (r = 4) or 17 (r = 2) mod 32 puts them on disjoint banks.
// weight: rows ci (the operand that takes the activation), columns (j, m) in one block of 16 m
//         per tap, K = (b, u) in chunks of 64 u; split and summed like the weight kernel above.
//         gbias: the taps with sh(j) = 1 cover each phase of the chunk's own r x 64 columns
//         exactly once, so the lanes sum the B fragments they feed the MFMAs: no pass over gy.
template <int R> struct Tc {
    static constexpr int K = 2 * R;
    __host__ __device__ static constexpr int q(int j) { return (j + R / 2) % R; }
    __host__ __device__ static constexpr int sh(int j) { return (j + R / 2) / R; }
};

constexpr int kTdCT = 32;          // ci rows per workgroup (two MFMA row blocks)
constexpr int kTdTN = 128;         // columns u per workgroup: 32 per wave (two column blocks)
constexpr int kTdMC = 16;          // output channels m per staged K chunk
constexpr int kTdPC = kTdTN + 2;   // window indices per phase
constexpr int td_pr(int r) { return r == 2 ? 145 : 144; }            // phase row stride
constexpr int td_wr(int r) { return kTdMC * 2 * r + 2; }             // weight row stride
static_assert(td_pr(4) % 32 == 16 && td_pr(2) % 32 == 17 && td_pr(2) >= kTdPC && td_pr(4) >= kTdPC, "window banks");
static_assert(td_wr(2) % 4 == 2 && td_wr(4) % 4 == 2, "weight rows: banks 2 row' + k");

template <int R>
__global__ __launch_bounds__(256) void convt1d_grad_data_kernel(CgArgs a) {
    using G = Tc<R>;
    constexpr int K = G::K, PR = td_pr(R), XR = R * PR, WR = td_wr(R), MK = kTdMC * K;
    __shared__ float gs[kTdMC * XR];                      // [m][phase][index]
    __shared__ float wsm[kTdCT * WR];                     // [ci][m][j]: W's rows as they are
    __shared__ float red[4 * kTdCT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = lane >> 4, col = lane & 15;
    const int b = blockIdx.z;
    const int u0 = blockIdx.x * kTdTN, ci0 = blockIdx.y * kTdCT;
    const bool want_alpha = a.act == RAVE_ACT_SNAKE && a.apart != nullptr;
    const float* gyb = a.gy + (int64_t)b * a.gy_sb;
    const int64_t tw0 = ((int64_t)u0 - 1) * R;            // t of window column 0
    int boff[K / 4];                                      // this lane's tap j = 4 jh + kk in the window
#pragma unroll
    for (int jh = 0; jh < K / 4; ++jh) {
        const int j = 4 * jh + kk;
        boff[jh] = ((j + R / 2) % R) * PR + (j + R / 2) / R + wave * 32 + col;
    }

    f32x4 acc[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int m0 = 0; m0 < a.c_out; m0 += kTdMC) {
        __syncthreads();
        {
            constexpr int NG = ceil_div(kTdMC * R * kTdPC, 256), NWI = kTdCT * MK / 256;
            float gv[NG], wv[NWI];
#pragma unroll
            for (int it = 0; it < NG; ++it) {
                const int e = tid + it * 256;
                const int m = e / (R * kTdPC), w = e - m * (R * kTdPC);
                const int64_t t = tw0 + w;
                const bool ok = m < kTdMC && m0 + m < a.c_out && t >= 0 && t < a.t_out;
                gv[it] = ok ? gyb[(int64_t)(m0 + m) * a.gy_sc + t] : 0.f;
            }
#pragma unroll
            for (int it = 0; it < NWI; ++it) {
                const int e = tid + it * 256;
                const int ci = e / MK, off = e - ci * MK;
                const bool ok = ci0 + ci < a.c_in && m0 + off / K < a.c_out;
                wv[it] = ok ? a.w[((int64_t)(ci0 + ci) * a.c_out + m0) * K + off] : 0.f;
            }
#pragma unroll
            for (int it = 0; it < NG; ++it) {
                const int e = tid + it * 256;
                const int m = e / (R * kTdPC), w = e - m * (R * kTdPC);
                if (m < kTdMC) gs[m * XR + (w % R) * PR + w / R] = gv[it];
            }
#pragma unroll
            for (int it = 0; it < NWI; ++it) {
                const int e = tid + it * 256;
                const int ci = e / MK, off = e - ci * MK;
                wsm[ci * WR + off] = wv[it];
            }
        }
        __syncthreads();
        const float* wa = wsm + col * WR + kk;
#pragma unroll 4
        for (int m = 0; m < kTdMC; ++m) {
#pragma unroll
            for (int jh = 0; jh < K / 4; ++jh) {
                const float a0 = wa[m * K + 4 * jh], a1 = wa[16 * WR + m * K + 4 * jh];
                const float b0 = gs[m * XR + boff[jh]], b1 = gs[m * XR + boff[jh] + 16];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    // D: row ci = 4 kk + r of the row block, column u = col of the column block
    const float* xb = a.x ? a.x + (int64_t)b * a.x_sb : nullptr;
    float* gxb = a.gx ? a.gx + (int64_t)b * a.gx_sb : nullptr;
    float asum[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = ci0 + rb * 16 + 4 * kk + r;
            const bool cok = ci < a.c_in;
            float al = 0.f, rr = 0.f;
            if (a.act == RAVE_ACT_SNAKE) {
                al = a.alpha[cok ? ci : 0];
                rr = 1.0f / (al + 1e-9f);
            }
            float sum = 0.f;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const int u = u0 + wave * 32 + cb * 16 + col;
                const bool ok = cok && u < a.t_in;
                const float ga = acc[rb][cb][r];
                float g = ga;
                if (a.act != RAVE_ACT_NONE) {
                    const float xv = ok ? xb[(int64_t)ci * a.x_sc + u] : 0.f;
                    if (a.act == RAVE_ACT_LEAKY) {
                        g = xv > 0.f ? ga : ga * a.slope;
                    } else {
                        float sin2, ssq;
                        snake_parts(al * xv, sin2, ssq);
                        g = ga * fmaf(al * rr, sin2, 1.0f);
                        const float da = (xv * sin2) * rr - (ssq * rr) * rr;
                        sum += ok ? ga * da : 0.f;
                    }
                }
                if (ok && gxb) gxb[(int64_t)ci * a.gx_sc + u] = g;
            }
            asum[rb][r] = sum;
        }
    }
    if (want_alpha) {                                     // uniform
        float* aprow = a.apart + ((int64_t)b * gridDim.x + blockIdx.x) * a.c_in;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = asum[rb][r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
                if (col == 0) red[wave * kTdCT + rb * 16 + 4 * kk + r] = v;
            }
        __syncthreads();
        if (tid < kTdCT && ci0 + tid < a.c_in)
            aprow[ci0 + tid] = ((red[tid] + red[kTdCT + tid]) + red[2 * kTdCT + tid]) + red[3 * kTdCT + tid];
    }
}

constexpr int kTwCT = 64;          // rows ci per workgroup: one MFMA row block per wave
constexpr int kTwMT = 16;          // output channels per workgroup: one column block per tap
constexpr int kTwTK = 64;          // input columns u per staged K chunk
constexpr int kTwXR = 66;          // input row stride: 2 x 33
constexpr int kTwPC = kTwTK + 2;   // window indices per phase
constexpr int tw_gr(int r) { return r * kTwPC + 2; }                 // gy row stride per m
static_assert(kTwXR % 4 == 2 && tw_gr(2) % 4 == 2 && tw_gr(4) % 4 == 2, "rows: banks 2 row' + k");

template <int R>
__global__ __launch_bounds__(256) void convt1d_grad_weight_kernel(CgArgs a) {
    using G = Tc<R>;
    constexpr int K = G::K, GR = tw_gr(R);
    __shared__ float xs[kTwCT * kTwXR];                   // [ci][u], act applied
    __shared__ float gys[kTwMT * GR];                     // [m][phase][index]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = lane >> 4, col = lane & 15;
    const int ci0 = blockIdx.x * kTwCT, m0 = blockIdx.y * kTwMT, sp = blockIdx.z;
    f32x4 acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const int ch_end = min((sp + 1) * a.cps, a.nch);
    for (int ch = sp * a.cps; ch < ch_end; ++ch) {
        const int b = ch / a.tch;
        const int u0 = (ch - b * a.tch) * kTwTK;
        const float* gyb = a.gy + (int64_t)b * a.gy_sb;
        const float* xb = a.x ? a.x + (int64_t)b * a.x_sb : nullptr;
        const int64_t tw0 = ((int64_t)u0 - 1) * R;        // t of window column 0
        __syncthreads();
        {
            constexpr int XT = kTwCT * kTwTK / 256, NG = ceil_div(kTwMT * R * kTwPC, 256);
            float xv[XT], gv[NG];
#pragma unroll
            for (int it = 0; it < XT; ++it) {
                const int e = tid + it * 256;
                const int ci = ci0 + (e >> 6), u = u0 + (e & 63);
                const bool ok = a.gw != nullptr && ci < a.c_in && u < a.t_in;     // bias only: x unread
                float v = ok ? xb[(int64_t)ci * a.x_sc + u] : 0.f;
                if (a.act != RAVE_ACT_NONE && ok)
                    v = apply_act(v, a.act, a.slope, a.act == RAVE_ACT_SNAKE ? a.alpha[ci] : 0.f);
                xv[it] = v;
            }
#pragma unroll
            for (int it = 0; it < NG; ++it) {
                const int e = tid + it * 256;
                const int m = e / (R * kTwPC), w = e - m * (R * kTwPC);
                const int64_t t = tw0 + w;
                const bool ok = m < kTwMT && m0 + m < a.c_out && t >= 0 && t < a.t_out;
                gv[it] = ok ? gyb[(int64_t)(m0 + m) * a.gy_sc + t] : 0.f;
            }
#pragma unroll
            for (int it = 0; it < XT; ++it) {
                const int e = tid + it * 256;
                xs[(e >> 6) * kTwXR + (e & 63)] = xv[it];
            }
#pragma unroll
            for (int it = 0; it < NG; ++it) {
                const int e = tid + it * 256;
                const int m = e / (R * kTwPC), w = e - m * (R * kTwPC);
                if (m < kTwMT) gys[m * GR + (w % R) * kTwPC + w / R] = gv[it];
            }
        }
        __syncthreads();
        const float* xa = xs + (wave * 16 + col) * kTwXR + kk;
        const float* gb = gys + col * GR + kk;
#pragma unroll 2
        for (int st = 0; st < kTwTK / 4; ++st) {
            const float av = xa[4 * st];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float bv = gb[G::q(j) * kTwPC + G::sh(j) + 4 * st];
                if (G::sh(j) == 1) bsum += bv;            // the chunk's own columns of phase q(j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
            }
        }
    }
    // D: row ci = 4 kk + r of this wave's row block, column m = col
    const int64_t WN = (int64_t)a.c_in * a.c_out * K;     // slab: the weights, then c_out bias sums
    const bool direct = a.S == 1;
    float* dst = direct ? a.gw : a.slabs + (int64_t)sp * (WN + a.c_out);
    const int m = m0 + col;
    if (a.gw && m < a.c_out) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = ci0 + wave * 16 + 4 * kk + r;
            if (ci >= a.c_in) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) dst[((int64_t)ci * a.c_out + m) * K + j] = acc[j][r];
        }
    }
    // gbias: this lane's B values are column `col`, k = kk: sum the four k lanes
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    if (blockIdx.x == 0 && wave == 0 && lane < 16 && m < a.c_out) {
        if (!direct)
            dst[WN + m] = bsum;
        else if (a.gb)
            a.gb[m] = bsum;
    }
}

// ---------------------------------------------------------------- host side
using BwdArgs = rave_conv1d_backward_args;

// The forward's refusals (conv_shared.h prepare_common) in its order, then this file's own.
static int check_args(const BwdArgs* p) {
    RAVE_CHECK_ARG(p, "conv1d_backward: null args");
    const BwdArgs& a = *p;
    RAVE_CHECK_ARG(a.precision == RAVE_PREC_F32, "conv1d_backward: precision must be RAVE_PREC_F32");
    RAVE_CHECK_ARG(a.batch > 0 && a.t_in > 0 && a.t_out > 0 && a.c_in > 0 && a.c_out > 0,
                   "conv1d_backward: empty shape");
    RAVE_CHECK_ARG(a.act != RAVE_ACT_SNAKE || a.alpha, "conv1d_backward: snake needs alpha");
    RAVE_CHECK_ARG(a.act >= RAVE_ACT_NONE && a.act <= RAVE_ACT_SNAKE, "conv1d_backward: unknown activation");
    RAVE_CHECK_ARG(a.pad_left >= 0 && a.pad_right >= 0, "conv1d_backward: negative padding");
    RAVE_CHECK_ARG(!a.transposed, "conv1d_backward: transposed convs have no backward yet");
    if (!family_supported(a.kernel) || a.kernel == 2 || family_stride(a.kernel) != a.stride) {
        set_error("conv1d_backward: unsupported (kernel, stride) pair; supported: k1/k3/k7 s1, k4 s2, k8 s4");
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(a.dilation == 1 || a.kernel == 3, "conv1d_backward: dilation only on 3-tap convs");
    RAVE_CHECK_ARG(a.dilation >= 1 && a.dilation <= kMaxDil, "conv1d_backward: dilation out of range");
    const int span = (a.kernel - 1) * a.dilation + 1;
    const int expect = (a.t_in + a.pad_left + a.pad_right - span) / a.stride + 1;
    RAVE_CHECK_ARG(expect == a.t_out, "conv1d_backward: t_out does not match the conv arithmetic");
    return RAVE_OK;
}

// transposed: the offline geometry only, strides 2 and 4
static int check_args_t(const BwdArgs* p) {
    RAVE_CHECK_ARG(p, "conv_transpose1d_backward: null args");
    const BwdArgs& a = *p;
    RAVE_CHECK_ARG(a.precision == RAVE_PREC_F32, "conv_transpose1d_backward: precision must be RAVE_PREC_F32");
    RAVE_CHECK_ARG(a.transposed == 1, "conv_transpose1d_backward: transposed must be 1 (rave_conv1d_backward_* takes the rest)");
    RAVE_CHECK_ARG(a.batch > 0 && a.t_in > 0 && a.t_out > 0 && a.c_in > 0 && a.c_out > 0,
                   "conv_transpose1d_backward: empty shape");
    RAVE_CHECK_ARG(a.act >= RAVE_ACT_NONE && a.act <= RAVE_ACT_SNAKE, "conv_transpose1d_backward: unknown activation");
    RAVE_CHECK_ARG(a.act != RAVE_ACT_SNAKE || a.alpha, "conv_transpose1d_backward: snake needs alpha");
    RAVE_CHECK_ARG(a.stride > 0 && a.kernel == 2 * a.stride, "conv_transpose1d_backward: kernel must be 2 * stride");
    RAVE_CHECK_ARG(a.pad_left == 0 && a.out_shift == a.stride / 2,
                   "conv_transpose1d_backward: only the offline geometry (pad_left = 0, out_shift = stride/2); the "
                   "cached form (pad_left = 1, out_shift = 0) has no backward");
    if (a.stride != 2 && a.stride != 4) {
        set_error("conv_transpose1d_backward: unsupported stride; supported: 2 and 4");
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG((int64_t)a.t_in * a.stride == a.t_out, "conv_transpose1d_backward: t_out must be t_in * stride");
    return RAVE_OK;
}

struct WgSplit {
    int S, cps, nch, tch;
};
// (the same split with and without gweight: gbias keeps its bits)  fill two workgroups per CU,
// each split at least four chunks (256 columns of K) long
static WgSplit weight_split(int chunks_per_row, int batch, int tiles) {
    WgSplit w;
    w.tch = chunks_per_row;
    w.nch = batch * w.tch;
    const int S = std::max(1, std::min(ceil_div(512, tiles), w.nch / 4));
    w.cps = ceil_div(w.nch, S);
    w.S = ceil_div(w.nch, w.cps);
    return w;
}

enum CgFamily { kFamConv, kFamConvT };

// A family's launches and workspace for one call.  A new family adds its name here, its checker, a
// function that fills name, data_z, the grids' x and y and the split from its tile constants, and
// its cases to the switches of make_plan, backward_data and backward_weight.
struct CgPlan {
    const char* name;             // the messages' prefix
    dim3 data_grid, weight_grid;  // data_grid.z is set from data_z once that is known to fit
    int64_t data_z;
    WgSplit split;
    int64_t slab_floats, alpha_floats;                    // the workspace: weight slabs, then alpha partial rows
};

static void plan_conv(const BwdArgs& a, CgPlan& pl) {
    pl.name = "conv1d_backward";
    pl.data_grid = dim3(ceil_div(ceil_div(a.t_in, a.stride), kDgTN), ceil_div(a.c_in, kDgCT));
    pl.data_z = (int64_t)a.batch * a.stride;
    const int mt = ceil_div(a.c_out, kWgMT), ct = ceil_div(a.c_in, kWgCT);
    pl.split = weight_split(ceil_div(a.t_out, kWgTK), a.batch, mt * ct);
    // bias only: one ci tile carries the row sums (x is not read, no weight is stored)
    pl.weight_grid = dim3(mt, a.gweight ? ct : 1);
}

static void plan_convt(const BwdArgs& a, CgPlan& pl) {
    pl.name = "conv_transpose1d_backward";
    pl.data_grid = dim3(ceil_div(a.t_in, kTdTN), ceil_div(a.c_in, kTdCT));
    pl.data_z = a.batch;
    const int ct = ceil_div(a.c_in, kTwCT), mt = ceil_div(a.c_out, kTwMT);
    pl.split = weight_split(ceil_div(a.t_in, kTwTK), a.batch, ct * mt);
    // bias only: one ci tile carries the column sums (x is not read, no weight is stored)
    pl.weight_grid = dim3(a.gweight ? ct : 1, mt);
}

static int make_plan(const BwdArgs* p, CgFamily fam, CgPlan& pl) {
    const int rc = fam == kFamConvT ? check_args_t(p) : check_args(p);
    if (rc != RAVE_OK) return rc;
    const BwdArgs& a = *p;
    switch (fam) {
        case kFamConv: plan_conv(a, pl); break;
        case kFamConvT: plan_convt(a, pl); break;
    }
    pl.weight_grid.z = pl.split.S;
    const bool slabs = (a.gweight || a.gbias) && pl.split.S > 1;
    pl.slab_floats = slabs ? (int64_t)pl.split.S * ((int64_t)a.c_in * a.c_out * a.kernel + a.c_out) : 0;
    const bool alpha = a.act == RAVE_ACT_SNAKE && a.galpha;
    pl.alpha_floats = alpha ? (int64_t)pl.data_grid.x * pl.data_z * a.c_in : 0;
    return RAVE_OK;
}

static CgArgs kernel_args(const BwdArgs& a, const CgPlan& pl) {
    CgArgs k{};
    k.x = a.x; k.gy = a.gy; k.w = a.weight; k.alpha = a.alpha;
    k.gx = a.gx; k.gw = a.gweight; k.gb = a.gbias; k.galpha = a.galpha;
    k.x_sb = a.x_sb; k.x_sc = a.x_sc; k.gy_sb = a.gy_sb; k.gy_sc = a.gy_sc; k.gx_sb = a.gx_sb; k.gx_sc = a.gx_sc;
    k.c_in = a.c_in; k.c_out = a.c_out; k.k = a.kernel; k.s = a.stride; k.d = a.dilation; k.pl = a.pad_left;
    k.t_in = a.t_in; k.t_out = a.t_out; k.B = a.batch; k.act = a.act; k.slope = a.leaky_slope;
    k.slabs = a.workspace;
    k.apart = pl.alpha_floats && a.workspace ? a.workspace + pl.slab_floats : nullptr;
    k.S = pl.split.S; k.cps = pl.split.cps; k.nch = pl.split.nch; k.tch = pl.split.tch;
    return k;
}

static int64_t backward_workspace(const BwdArgs* p, CgFamily fam) {
    CgPlan pl;
    const int rc = make_plan(p, fam, pl);
    return rc != RAVE_OK ? rc : pl.slab_floats + pl.alpha_floats;
}

static int backward_data(const BwdArgs* p, void* stream, CgFamily fam) {
    CgPlan pl;
    const int rc = make_plan(p, fam, pl);
    if (rc != RAVE_OK) return rc;
    const BwdArgs& a = *p;
    const bool want_alpha = pl.alpha_floats > 0;
    if (!a.gx && !want_alpha) return RAVE_OK;
    const auto msg = [&](const char* what) { return std::string(pl.name) + "_data: " + what; };
    RAVE_CHECK_ARG(a.gy && a.weight, msg("null gy or weight"));
    RAVE_CHECK_ARG(a.act == RAVE_ACT_NONE || a.x, msg("the activation's derivative needs the input x"));
    RAVE_CHECK_ARG(!want_alpha || a.workspace, msg("galpha needs the workspace"));
    RAVE_CHECK_ARG(pl.data_grid.y <= 65535 && pl.data_z <= 65535, msg("grid beyond 65535 in y or z"));
    const dim3 grid(pl.data_grid.x, pl.data_grid.y, (unsigned)pl.data_z);
    CgArgs k = kernel_args(a, pl);
    k.P = (int)(grid.x * grid.z);
    hipStream_t st = as_stream(stream);
    const char* kernel = "conv1d_grad_data_kernel";
    switch (fam) {
        case kFamConv: launch(conv1d_grad_data_kernel, grid, dim3(256), 0, st, k); break;
        case kFamConvT:
            kernel = "convt1d_grad_data_kernel";
            if (a.stride == 2)
                launch(convt1d_grad_data_kernel<2>, grid, dim3(256), 0, st, k);
            else
                launch(convt1d_grad_data_kernel<4>, grid, dim3(256), 0, st, k);
            break;
    }
    const int s = launch_status(kernel);
    if (s != RAVE_OK || !want_alpha) return s;
    launch(conv1d_grad_alpha_reduce_kernel, dim3(a.c_in), dim3(64), 0, st, k);
    return launch_status("conv1d_grad_alpha_reduce_kernel");
}

static int backward_weight(const BwdArgs* p, void* stream, CgFamily fam) {
    CgPlan pl;
    const int rc = make_plan(p, fam, pl);
    if (rc != RAVE_OK) return rc;
    const BwdArgs& a = *p;
    if (!a.gweight && !a.gbias) return RAVE_OK;
    const auto msg = [&](const char* what) { return std::string(pl.name) + "_weight: " + what; };
    RAVE_CHECK_ARG(a.gy, msg("null gy"));
    RAVE_CHECK_ARG(a.x || !a.gweight, msg("gweight needs the input x"));
    RAVE_CHECK_ARG(pl.split.S == 1 || a.workspace, msg("the K split needs the workspace"));
    const dim3 grid = pl.weight_grid;
    RAVE_CHECK_ARG(grid.y <= 65535 && grid.z <= 65535, msg("grid beyond 65535 in y or z"));
    const CgArgs k = kernel_args(a, pl);
    hipStream_t st = as_stream(stream);
    const char* kernel = "conv1d_grad_weight_kernel";
    switch (fam) {
        case kFamConv:
            switch (a.kernel) {
                case 1: launch(conv1d_grad_weight_kernel<1>, grid, dim3(256), 0, st, k); break;
                case 3: launch(conv1d_grad_weight_kernel<3>, grid, dim3(256), 0, st, k); break;
                case 7: launch(conv1d_grad_weight_kernel<7>, grid, dim3(256), 0, st, k); break;
                case 4: launch(conv1d_grad_weight_kernel<4>, grid, dim3(256), 0, st, k); break;
                default: launch(conv1d_grad_weight_kernel<8>, grid, dim3(256), 0, st, k); break;
            }
            break;
        case kFamConvT:
            kernel = "convt1d_grad_weight_kernel";
            if (a.stride == 2)
                launch(convt1d_grad_weight_kernel<2>, grid, dim3(256), 0, st, k);
            else
                launch(convt1d_grad_weight_kernel<4>, grid, dim3(256), 0, st, k);
            break;
    }
    const int s = launch_status(kernel);
    if (s != RAVE_OK || pl.split.S == 1) return s;
    const int64_t total = (int64_t)a.c_in * a.c_out * a.kernel + a.c_out;
    const dim3 rgrid((unsigned)std::min<int64_t>(1024, ceil_div64(total, 256)));
    launch(grad_slab_reduce_kernel, rgrid, dim3(256), 0, st, k);
    return launch_status("grad_slab_reduce_kernel");
}

}  // namespace rave

using namespace rave;

extern "C" int64_t rave_conv1d_backward_workspace(const BwdArgs* p) { return backward_workspace(p, kFamConv); }
extern "C" int rave_conv1d_backward_data(const BwdArgs* p, void* stream) { return backward_data(p, stream, kFamConv); }
extern "C" int rave_conv1d_backward_weight(const BwdArgs* p, void* stream) {
    return backward_weight(p, stream, kFamConv);
}
extern "C" int64_t rave_conv_transpose1d_backward_workspace(const BwdArgs* p) {
    return backward_workspace(p, kFamConvT);
}
extern "C" int rave_conv_transpose1d_backward_data(const BwdArgs* p, void* stream) {
    return backward_data(p, stream, kFamConvT);
}
extern "C" int rave_conv_transpose1d_backward_weight(const BwdArgs* p, void* stream) {
    return backward_weight(p, stream, kFamConvT);
}
