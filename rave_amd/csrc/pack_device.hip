// rave_conv1d_pack_weight on the device: the exact-fp32 packed image of a conv
// weight (conv1d.hip's layout) written from the torch-layout weight in device
// memory, so that a training step's weight update never goes through the host.
//
// The image is nchunks * BK rows of Mpad floats (BK = taps * CIT, Mpad = rows
// padded to 128); row (c, j, cl) holds tap j of input channel ci = c * CIT + cl
// for every GEMM row m.  Both kernels are permutation copies and write every
// float of rave_conv1d_packed_size(): the rows of channels past c_in, the
// columns past the last GEMM row and, transposed, the group-0 padding rows and
// the tail up to the larger of the two row layouts are stored as zeros, so the
// destination needs no clearing.  Plain vector loads and stores, no atomics.
//
//  * Conv1d: packed[r(e)][m] = w[m][e] with e = ci * k + j, a transpose.  A
//    workgroup moves a 64 (m) x 64 (e) tile through LDS: each wave reads runs of
//    64 consecutive e of one m (256 contiguous bytes of w), stores them as one
//    row of the tile, and after the barrier reads columns of the tile and writes
//    64 consecutive m of one image row (256 contiguous bytes).  The tile's row
//    stride is 65 floats: ds_write_b32 / ds_read_b32 bank a 32-lane half's
//    addresses mod 32; the stores walk e (32 consecutive floats), the loads walk
//    m at stride 65 = 1 mod 32, so both sides touch 32 distinct banks.
//  * ConvTranspose1d: row m <-> (co, q) reads w[ci][co][kidx(j, q)]; for one ci
//    both taps together read the span of c_out * 2r floats exactly once, so a
//    wave's 64 consecutive m read one contiguous stretch of it: no transpose.
//    One workgroup per image row.
#include "conv_shared.h"

namespace rave {

constexpr int kPackTile = 64;
constexpr int kPackLds = kPackTile + 1;   // row stride in floats (1 mod 32)

struct PackArgs {
    const float* w;
    float* packed;
    int c_in, c_out, kernel, cit, taps;
    int M, Mpad, rows;            // GEMM rows, padded rows, image rows (nchunks * taps * cit)
    int R, q0, split_row, out_shift;
    int tail;                     // transposed: floats per image row between this layout and the larger one
};

// image row of e = ci * k + j (ci may run past c_in, up to nchunks * cit: a zero row)
__device__ __forceinline__ int pack_row(const PackArgs& a, int e) {
    const int ci = e / a.kernel, j = e - ci * a.kernel;
    const int c = ci / a.cit, cl = ci - c * a.cit;
    return (c * a.taps + j) * a.cit + cl;
}

__global__ __launch_bounds__(256) void pack_conv_kernel(PackArgs a) {
    __shared__ float tile[kPackTile * kPackLds];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e0 = blockIdx.x * kPackTile, m0 = blockIdx.y * kPackTile;
    const int E = a.c_in * a.kernel;              // floats of one weight row
    // w[m][e0 + lane] for the wave's 16 rows: all loads in flight before the first LDS store
    float v[kPackTile / 4];
    const int e = e0 + lane;
#pragma unroll
    for (int i = 0; i < kPackTile / 4; ++i) {
        const int m = m0 + wave + 4 * i;
        v[i] = (m < a.c_out && e < E) ? a.w[(int64_t)m * E + e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kPackTile / 4; ++i) tile[(wave + 4 * i) * kPackLds + lane] = v[i];
    __syncthreads();
    // image row r(e0 + el), columns m0 .. m0 + 63 (Mpad is a multiple of the tile)
#pragma unroll
    for (int i = 0; i < kPackTile / 4; ++i) {
        const int el = wave + 4 * i;
        if (e0 + el >= a.rows) break;             // rows = the e of every chunk, whole chunks
        const int r = pack_row(a, e0 + el);
        a.packed[(int64_t)r * a.Mpad + m0 + lane] = tile[lane * kPackLds + el];
    }
}

__global__ __launch_bounds__(256) void pack_convt_kernel(PackArgs a) {
    const int r = blockIdx.x;                     // image row (c, j, cl)
    const int c = r / (a.taps * a.cit), rr = r - c * (a.taps * a.cit);
    const int j = rr / a.cit, ci = c * a.cit + (rr - j * a.cit);
    const int p = a.R - a.q0;                     // phases in row group 1 (0: none)
    float* row = a.packed + (int64_t)r * a.Mpad;
    const float* src = a.w + (int64_t)ci * a.c_out * a.kernel;
    for (int m = threadIdx.x; m < a.Mpad; m += 256) {
        int co = a.c_out, q = 0;                  // padding unless a phase group claims the row
        if (m < a.split_row) {
            co = m / a.q0;
            q = m - co * a.q0;
        } else if (m < a.M) {                     // (M > split_row only when p > 0)
            const int mm = m - a.split_row;
            co = mm / p;
            q = a.q0 + (mm - co * p);
        }
        float v = 0.f;
        if (co < a.c_out && ci < a.c_in) {
            // output t = u*R + q: q < q0 reads taps (u-1, u), q >= q0 taps (u, u+1)
            const int first = q < a.q0 ? a.R : 0;       // the earlier tap's (j = 0) offset; j = 1 is R less
            v = src[co * a.kernel + q + a.out_shift + first - j * a.R];
        }
        row[m] = v;
    }
    // this row's share of the floats between this layout's end and packed_size
    float* tail = a.packed + (int64_t)a.rows * a.Mpad + (int64_t)r * a.tail;
    for (int i = threadIdx.x; i < a.tail; i += 256) tail[i] = 0.f;
}

}  // namespace rave

using namespace rave;

extern "C" int rave_conv1d_pack_weight_device(const float* w, int c_in, int c_out, int kernel, int stride,
                                              int dilation, int transposed, int out_shift, float* packed,
                                              void* stream) {
    // rave_conv1d_pack_weight's refusals, in its order; nothing before them touches the GPU
    RAVE_CHECK_ARG(w && packed, "pack_weight_device: null pointer");
    RAVE_CHECK_ARG(c_in > 0 && c_out > 0 && kernel > 0 && stride > 0 && dilation > 0,
                   "pack_weight_device: bad shape");
    const int ci_t = rave_conv1d_chunk(c_in, kernel, stride, dilation, transposed);
    if (ci_t <= 0) {
        set_error("pack_weight_device: unsupported layer shape");
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(!transposed || out_shift == 0 || out_shift == stride / 2,
                   "pack_weight_device: transposed out_shift must be 0 or stride/2");
    PackArgs a{};
    a.w = w; a.packed = packed;
    a.c_in = c_in; a.c_out = c_out; a.kernel = kernel; a.cit = ci_t;
    a.taps = transposed ? 2 : kernel;
    a.R = transposed ? stride : 1;
    a.out_shift = transposed ? out_shift : 0;
    a.q0 = a.R - a.out_shift;
    a.split_row = transposed ? convt_group1_row(c_out, a.R, a.q0) : 1 << 30;
    a.M = transposed ? a.split_row + c_out * (a.R - a.q0) : c_out;
    a.Mpad = ceil_div(a.M, 128) * 128;
    a.rows = ceil_div(c_in, ci_t) * ci_t * a.taps;
    hipStream_t st = as_stream(stream);
    if (transposed) {
        const int64_t total = rave_conv1d_packed_size(c_in, c_out, kernel, stride, dilation, transposed);
        a.tail = (int)(total / a.rows) - a.Mpad;          // both layouts have `rows` rows
        launch(pack_convt_kernel, dim3(a.rows), dim3(256), 0, st, a);
        return launch_status("pack_convt_kernel");
    }
    launch(pack_conv_kernel, dim3(ceil_div(a.rows, kPackTile), a.Mpad / kPackTile), dim3(256), 0, st, a);
    return launch_status("pack_conv_kernel");
}
