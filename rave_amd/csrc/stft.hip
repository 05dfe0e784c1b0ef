// Multi-scale STFT magnitudes and the spectral audio distance
// (core.MultiScaleSTFT / core.AudioDistanceV1, rave/core.py:278-353; the metric
// of RAVE.validation_step, rave/model.py:636-686).
//
// The transform is an LDS-resident complex fp32 FFT, radix-4 Stockham stages
// (plus one radix-2 stage when log2 n is odd) run in place: every thread reads
// its butterflies' inputs into registers, the workgroup meets at a barrier, and
// the outputs go back to the same arrays in the autosort order.  Real and
// imaginary parts live in separate arrays, so a stage's reads are unit-stride.
// One workgroup (256 threads) transforms kConc = max(1, 1024 / n) frames at
// once -- one radix-4 butterfly per thread for n <= 1024, 2 and 4 for n = 2048
// and 4096 -- and walks a tile of consecutive frames of one row in passes.
//
// Two real frames share one complex FFT (z = a + i b; A[k] = (Z[k] + conj
// Z[n-k]) / 2, B[k] = (Z[k] - conj Z[n-k]) / 2i).  The distance kernel pairs
// frame f of x with frame f of y and reduces |X|, |Y| to three sums per
// workgroup on the spot; the magnitude kernel pairs frames 2i and 2i+1 of one
// row.  Window and twiddles come from the caller's packed table (float64 on the
// host, rounded once); the reflect padding is an index computation at load.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "stft_fft.h"

namespace rave {
namespace {

// ------------------------------------------------------------------ distance
struct DistParams {
    const float* x;
    const float* y;
    const float* table[RAVE_STFT_MAX_SCALES];
    float* ws;                                   // 4 floats per workgroup
    int n[RAVE_STFT_MAX_SCALES];
    int frames[RAVE_STFT_MAX_SCALES];
    int tiles[RAVE_STFT_MAX_SCALES];             // frame tiles per row
    int blk0[RAVE_STFT_MAX_SCALES + 1];          // first workgroup of each scale
    int rows, t_len, n_scales;
    float eps;
};

template <int N>
__device__ __forceinline__ void distance_tile(const DistParams& p, int sc, int local, float* lds, float& sd,
                                              float& sx, float& sl) {
    using G = Geo<N>;
    constexpr int H = N / 2;
    float* re = lds;
    float* im = lds + G::kConc * N;
    // nz[2c], nz[2c + 1]: x's / y's frame in slot c has a nonzero sample (see
    // stft_mag_kernel: a frame of zeros has the spectrum 0, not its partner's noise)
    __shared__ int nz[2 * G::kConc];
    const float* win = p.table[sc];
    const float2* tw = reinterpret_cast<const float2*>(win + N);
    const int frames = p.frames[sc];
    const int row = local / p.tiles[sc];
    const int f_tile = (local % p.tiles[sc]) * G::kTile;
    const float* xr = p.x + (int64_t)row * p.t_len;
    const float* yr = p.y + (int64_t)row * p.t_len;
    for (int pass = 0; pass < G::kPasses; ++pass) {
        const int f0 = f_tile + pass * G::kConc;
        if (f0 >= frames) break;                                  // uniform over the workgroup
        if (threadIdx.x < 2 * G::kConc) nz[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < G::kConc * N / kThreads; ++u) {
            const int e = threadIdx.x + u * kThreads;
            const int f = f0 + e / N, j = e % N;
            float a = 0.f, b = 0.f;
            if (f < frames) {
                const int i = reflect(f * (N / 4) + j - H, p.t_len);
                const float w = win[j];
                a = w * xr[i];
                b = w * yr[i];
            }
            re[e] = a;
            im[e] = b;
            if (a != 0.f) nz[2 * (e / N)] = 1;                      // every writer stores the same 1
            if (b != 0.f) nz[2 * (e / N) + 1] = 1;
        }
        __syncthreads();
        fft_lds<N>(re, im, tw);
#pragma unroll
        for (int u = 0; u < G::kConc * H / kThreads; ++u) {
            const int e = threadIdx.x + u * kThreads;
            const int c = e / H, k = e % H;
            if (f0 + c >= frames) continue;
            const float* zr = re + c * N;
            const float* zi = im + c * N;
            const bool xz = nz[2 * c] == 0, yz = nz[2 * c + 1] == 0;
            float mx, my;
            if (k == 0) {
                // DC and Nyquist are their own mirror: X = Re Z, Y = Im Z
                mx = fabsf(zr[0]);
                my = fabsf(zi[0]);
                const float nx = xz ? 0.f : fabsf(zr[H]), ny = yz ? 0.f : fabsf(zi[H]);
                const float d = nx - ny;
                sd += d * d;
                sx += nx * nx;
                sl += fabsf(logf(nx + p.eps) - logf(ny + p.eps));
            } else {
                const float ar = zr[k], ai = zi[k], br = zr[N - k], bi = zi[N - k];
                const float xre = ar + br, xim = ai - bi;         // 2 X[k]
                const float yre = ai + bi, yim = br - ar;         // 2 Y[k]
                mx = 0.5f * sqrtf(xre * xre + xim * xim);
                my = 0.5f * sqrtf(yre * yre + yim * yim);
            }
            if (xz) mx = 0.f;
            if (yz) my = 0.f;
            const float d = mx - my;
            sd += d * d;
            sx += mx * mx;
            sl += fabsf(logf(mx + p.eps) - logf(my + p.eps));
        }
        __syncthreads();                                          // the next pass overwrites re / im
    }
}

__global__ __launch_bounds__(kThreads) void distance_kernel(DistParams p) {
    extern __shared__ float lds[];
    __shared__ float red[3 * kWaves];
    const int blk = blockIdx.x;
    int sc = 0;
    while (sc + 1 < p.n_scales && blk >= p.blk0[sc + 1]) ++sc;
    const int local = blk - p.blk0[sc];
    float sd = 0.f, sx = 0.f, sl = 0.f;
    switch (p.n[sc]) {
        case 64: distance_tile<64>(p, sc, local, lds, sd, sx, sl); break;
        case 128: distance_tile<128>(p, sc, local, lds, sd, sx, sl); break;
        case 256: distance_tile<256>(p, sc, local, lds, sd, sx, sl); break;
        case 512: distance_tile<512>(p, sc, local, lds, sd, sx, sl); break;
        case 1024: distance_tile<1024>(p, sc, local, lds, sd, sx, sl); break;
        case 2048: distance_tile<2048>(p, sc, local, lds, sd, sx, sl); break;
        default: distance_tile<4096>(p, sc, local, lds, sd, sx, sl); break;
    }
    sd = wave_sum(sd);
    sx = wave_sum(sx);
    sl = wave_sum(sl);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w] = sd;
        red[kWaves + w] = sx;
        red[2 * kWaves + w] = sl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {                        // fixed order
            a += red[i];
            b += red[kWaves + i];
            c += red[2 * kWaves + i];
        }
        float* slot = p.ws + (int64_t)blk * 4;
        slot[0] = a;
        slot[1] = b;
        slot[2] = c;
        slot[3] = 0.f;
    }
}

// One workgroup: per scale, every thread adds the slots t, t + 256, ... in
// double, then a fixed-order tree over the workgroup.
__global__ __launch_bounds__(kThreads) void distance_finalize_kernel(DistParams p, float* out) {
    __shared__ double red[3][kThreads];
    double total = 0.0;
    for (int sc = 0; sc < p.n_scales; ++sc) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int i = p.blk0[sc] + threadIdx.x; i < p.blk0[sc + 1]; i += kThreads) {
            const float* slot = p.ws + (int64_t)i * 4;
            a += (double)slot[0];
            b += (double)slot[1];
            c += (double)slot[2];
        }
        red[0][threadIdx.x] = a;
        red[1][threadIdx.x] = b;
        red[2][threadIdx.x] = c;
        __syncthreads();
        for (int h = kThreads / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) {
                red[0][threadIdx.x] += red[0][threadIdx.x + h];
                red[1][threadIdx.x] += red[1][threadIdx.x + h];
                red[2][threadIdx.x] += red[2][threadIdx.x + h];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const double count = (double)p.rows * (double)(p.n[sc] / 2 + 1) * (double)p.frames[sc];
            const double lin = red[0][0] / red[1][0];
            const double lg = red[2][0] / count;
            out[1 + 2 * sc] = (float)lin;
            out[2 + 2 * sc] = (float)lg;
            total += lin + lg;
        }
        __syncthreads();                                          // red is reused by the next scale
    }
    if (threadIdx.x == 0) out[0] = (float)total;
}

// ------------------------------------------------------------------ magnitudes
// grid (pair tiles, rows): transform c of a pass carries frames 2c and 2c + 1
// of the pass's 2 kConc frames.
template <int N>
__global__ __launch_bounds__(kThreads) void stft_mag_kernel(rave_stft_args a, int frames) {
    using G = Geo<N>;
    constexpr int H = N / 2;
    __shared__ float re[G::kConc * N];
    __shared__ float im[G::kConc * N];
    // nz[2c], nz[2c + 1]: frame 2c / 2c + 1 of the pass has a nonzero sample.  A
    // frame of zeros transforms to zeros; read back out of the shared FFT it would
    // come out as its partner's rounding noise instead.
    __shared__ int nz[2 * G::kConc];
    const float* win = a.table;
    const float2* tw = reinterpret_cast<const float2*>(win + N);
    const int row = blockIdx.y;
    const float* xr = a.x + (int64_t)row * a.t_len;
    float* yr = a.y + (int64_t)row * (H + 1) * frames;
    for (int pass = 0; pass < G::kPasses; ++pass) {
        const int f0 = 2 * (blockIdx.x * G::kTile + pass * G::kConc);
        if (f0 >= frames) break;
        if (threadIdx.x < 2 * G::kConc) nz[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < G::kConc * N / kThreads; ++u) {
            const int e = threadIdx.x + u * kThreads;
            const int fa = f0 + 2 * (e / N), j = e % N;
            const float w = win[j];
            float va = 0.f, vb = 0.f;
            if (fa < frames) va = w * xr[reflect(fa * (N / 4) + j - H, a.t_len)];
            if (fa + 1 < frames) vb = w * xr[reflect((fa + 1) * (N / 4) + j - H, a.t_len)];
            re[e] = va;
            im[e] = vb;
            if (va != 0.f) nz[2 * (e / N)] = 1;                     // every writer stores the same 1
            if (vb != 0.f) nz[2 * (e / N) + 1] = 1;
        }
        __syncthreads();
        fft_lds<N>(re, im, tw);
#pragma unroll
        for (int u = 0; u < G::kConc * H / kThreads; ++u) {
            const int e = threadIdx.x + u * kThreads;
            const int c = e / H, k = e % H;
            const int fa = f0 + 2 * c;
            if (fa >= frames) continue;
            const bool second = fa + 1 < frames;
            const float* zr = re + c * N;
            const float* zi = im + c * N;
            const bool za = nz[2 * c] == 0, zb = nz[2 * c + 1] == 0;
            float ma, mb;
            if (k == 0) {
                ma = fabsf(zr[0]);
                mb = fabsf(zi[0]);
                yr[(int64_t)H * frames + fa] = za ? 0.f : fabsf(zr[H]);
                if (second) yr[(int64_t)H * frames + fa + 1] = zb ? 0.f : fabsf(zi[H]);
            } else {
                const float ar = zr[k], ai = zi[k], br = zr[N - k], bi = zi[N - k];
                const float are = ar + br, aim = ai - bi;
                const float bre = ai + bi, bim = br - ar;
                ma = 0.5f * sqrtf(are * are + aim * aim);
                mb = 0.5f * sqrtf(bre * bre + bim * bim);
            }
            yr[(int64_t)k * frames + fa] = za ? 0.f : ma;
            if (second) yr[(int64_t)k * frames + fa + 1] = zb ? 0.f : mb;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ host

// Validation shared by the workspace query and the op (pointers excluded).
int check_distance_shape(const rave_distance_args* a, DistParams* p) {
    RAVE_CHECK_ARG(a != nullptr, "audio_distance: null arguments");
    if (a->n_scales < 1 || a->n_scales > RAVE_STFT_MAX_SCALES) {
        set_error("audio_distance: 1 to " + std::to_string(RAVE_STFT_MAX_SCALES) + " scales per call, got " +
                  std::to_string(a->n_scales));
        return RAVE_ERR_UNSUPPORTED;
    }
    int max_n = 0;
    for (int s = 0; s < a->n_scales; ++s) {
        if (!scale_supported(a->scales[s])) {
            set_error("audio_distance: scale " + std::to_string(a->scales[s]) +
                      " is not a power of two in [64, 4096]");
            return RAVE_ERR_UNSUPPORTED;
        }
        max_n = std::max(max_n, a->scales[s]);
    }
    RAVE_CHECK_ARG(a->rows > 0 && a->t_len > 0, "audio_distance: rows and t_len must be positive");
    RAVE_CHECK_ARG(a->t_len > max_n / 2, "audio_distance: reflect padding needs t_len > max(scales) / 2");
    RAVE_CHECK_ARG(a->t_len <= (1 << 30), "audio_distance: t_len above 2^30");
    RAVE_CHECK_ARG(std::isfinite(a->log_epsilon) && a->log_epsilon > 0.f,
                   "audio_distance: log_epsilon must be positive");
    int64_t blocks = 0;
    for (int s = 0; s < a->n_scales; ++s) {
        const int n = a->scales[s];
        const int frames = 1 + a->t_len / (n / 4);
        const int tiles = ceil_div(frames, tile_of(n));
        p->n[s] = n;
        p->frames[s] = frames;
        p->tiles[s] = tiles;
        p->blk0[s] = (int)blocks;
        blocks += (int64_t)a->rows * tiles;
        RAVE_CHECK_ARG(blocks < (1LL << 30), "audio_distance: rows * frames too large for one launch");
    }
    p->blk0[a->n_scales] = (int)blocks;
    p->rows = a->rows;
    p->t_len = a->t_len;
    p->n_scales = a->n_scales;
    p->eps = a->log_epsilon;
    return RAVE_OK;
}

template <int N>
void launch_mag(const rave_stft_args& a, int frames, hipStream_t st) {
    const int pairs = ceil_div(frames, 2);
    launch(stft_mag_kernel<N>, dim3(ceil_div(pairs, Geo<N>::kTile), a.rows), dim3(kThreads), 0, st, a, frames);
}

}  // namespace
}  // namespace rave

using namespace rave;

extern "C" int64_t rave_stft_table_size(int n) {
    if (!scale_supported(n)) {
        set_error("stft_table_size: scale " + std::to_string(n) + " is not a power of two in [64, 4096]");
        return -1;
    }
    return 3 * (int64_t)n;
}

extern "C" int rave_stft_pack_table(int n, float* out) {
    if (!scale_supported(n)) {
        set_error("stft_pack_table: scale " + std::to_string(n) + " is not a power of two in [64, 4096]");
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(out != nullptr, "stft_pack_table: null output");
    const double step = 2.0 * 3.14159265358979323846 / (double)n;
    for (int i = 0; i < n; ++i) {
        out[i] = (float)(0.5 - 0.5 * std::cos(step * i));
        out[n + 2 * i] = (float)std::cos(step * i);
        out[n + 2 * i + 1] = (float)(-std::sin(step * i));
    }
    return RAVE_OK;
}

extern "C" int rave_stft_mag(const rave_stft_args* a, void* stream) {
    RAVE_CHECK_ARG(a != nullptr, "stft_mag: null arguments");
    if (!scale_supported(a->n)) {
        set_error("stft_mag: scale " + std::to_string(a->n) + " is not a power of two in [64, 4096]");
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(a->rows > 0 && a->rows <= 65535, "stft_mag: rows must be in [1, 65535]");
    RAVE_CHECK_ARG(a->t_len > a->n / 2, "stft_mag: reflect padding needs t_len > n / 2");
    RAVE_CHECK_ARG(a->t_len <= (1 << 30), "stft_mag: t_len above 2^30");
    RAVE_CHECK_ARG(a->x && a->table && a->y, "stft_mag: null x, table or y");
    const int frames = 1 + a->t_len / (a->n / 4);
    hipStream_t st = as_stream(stream);
    switch (a->n) {
        case 64: launch_mag<64>(*a, frames, st); break;
        case 128: launch_mag<128>(*a, frames, st); break;
        case 256: launch_mag<256>(*a, frames, st); break;
        case 512: launch_mag<512>(*a, frames, st); break;
        case 1024: launch_mag<1024>(*a, frames, st); break;
        case 2048: launch_mag<2048>(*a, frames, st); break;
        default: launch_mag<4096>(*a, frames, st); break;
    }
    return launch_status("stft_mag");
}

extern "C" int64_t rave_audio_distance_workspace(const rave_distance_args* a) {
    DistParams p;
    if (check_distance_shape(a, &p) != RAVE_OK) return -1;
    return (int64_t)p.blk0[p.n_scales] * 4 * (int64_t)sizeof(float);
}

extern "C" int rave_audio_distance(const rave_distance_args* a, void* stream) {
    DistParams p;
    const int rc = check_distance_shape(a, &p);
    if (rc != RAVE_OK) return rc;
    RAVE_CHECK_ARG(a->x && a->y && a->workspace && a->out, "audio_distance: null x, y, workspace or out");
    size_t lds = 0;
    for (int s = 0; s < a->n_scales; ++s) {
        RAVE_CHECK_ARG(a->tables[s] != nullptr, "audio_distance: null table for scale " + std::to_string(a->scales[s]));
        p.table[s] = a->tables[s];
        lds = std::max(lds, lds_bytes_of(a->scales[s]));
    }
    p.x = a->x;
    p.y = a->y;
    p.ws = a->workspace;
    hipStream_t st = as_stream(stream);
    launch(distance_kernel, dim3(p.blk0[p.n_scales]), dim3(kThreads), (uint32_t)lds, st, p);
    int lrc = launch_status("audio_distance");
    if (lrc != RAVE_OK) return lrc;
    launch(distance_finalize_kernel, dim3(1), dim3(kThreads), 0, st, p, a->out);
    return launch_status("audio_distance finalize");
}
