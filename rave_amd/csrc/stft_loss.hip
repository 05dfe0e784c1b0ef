// The spectral training losses and their gradient with respect to the value
// signal: MultiResolutionSTFTLoss (rave/stft_loss.py:12-144, the criterion of
// RAVE.training_step, rave/model.py:191-198, 386-391) and AudioDistanceV1
// (rave/core.py:339-353).  The first backward kernel of the library.
//
// Forward: the structure of the distance kernel (stft.hip) with a general frame
// geometry (n_fft, hop, win <= n_fft: torch.stft's zero-padded, centred window).
// Frame f of the value is the real and frame f of the target the imaginary part
// of one complex FFT; every workgroup reduces its bins to three partial sums in
// its own workspace slot and a one-workgroup finalize adds them in double in a
// fixed order.  Finalize also leaves the sums and the two loss derivatives per
// resolution in `saved` for the backward.
//
// Backward, per frame: redo the FFT, form G_k = (dL/d|V_k|) V_k / |V_k| for the
// one-sided bins in place (zero above n/2), run the same FFT on conj G -- the
// real part of FFT(conj G) is the real part of the unnormalised inverse DFT of
// G, so one twiddle table serves both directions -- and write the windowed
// samples of the frame to the workspace.  A gather kernel then sums, per output
// sample, the frames that cover it and its (at most two) reflect images in a
// fixed order: resolution, image (direct, left, right), frame index.  No
// atomics anywhere, so reruns are bitwise identical.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "stft_fft.h"

namespace rave {
namespace {

constexpr float kPowerClamp = 1e-7f;             // stft_loss.py:35

struct LossParams {
    const float* value;
    const float* target;
    const float* table[RAVE_STFT_MAX_SCALES];
    float* slots;                                // 4 floats per workgroup
    float* frames_ws;                            // backward: (rows, frames, win) per resolution
    const float* saved;
    const float* grad_out;
    float* grad_value;
    int64_t ws0[RAVE_STFT_MAX_SCALES];           // first float of each resolution in frames_ws
    int n[RAVE_STFT_MAX_SCALES];
    int hop[RAVE_STFT_MAX_SCALES];
    int win[RAVE_STFT_MAX_SCALES];
    int frames[RAVE_STFT_MAX_SCALES];
    int tiles[RAVE_STFT_MAX_SCALES];             // frame tiles per row
    int blk0[RAVE_STFT_MAX_SCALES + 1];          // first workgroup of each resolution
    int rows, t_len, n_res, kind;
    float eps;
};

// One bin: pv / pt are the powers of the value and the target.  Forward: adds
// the bin to the three sums.  Backward: returns (dL/d mag) / mag, the factor of
// the value's spectrum in G (c_lin / c_log carry the upstream gradients).
template <bool BWD>
__device__ __forceinline__ float bin_term(bool multires, float eps, float pv, float pt, float c_lin, float c_log,
                                          float& sd, float& st, float& sl) {
    float vm, tm, lv;                            // magnitudes; lv: the argument of the value's log
    if (multires) {
        vm = sqrtf(fmaxf(pv, kPowerClamp));
        tm = sqrtf(fmaxf(pt, kPowerClamp));
        lv = vm;
    } else {
        vm = sqrtf(pv);
        tm = sqrtf(pt);
        lv = vm + eps;
    }
    const float d = tm - vm;
    if (!BWD) {
        sd += d * d;
        st += tm * tm;
        sl += fabsf(logf(multires ? tm : tm + eps) - logf(lv));
        return 0.f;
    }
    // the clamp's derivative (multires) / torch's abs of a complex zero (V1)
    if (multires ? pv < kPowerClamp : vm == 0.f) return 0.f;
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);     // sign(log t - log v)
    const float w = -(d * c_lin) - sg * c_log / lv;
    return w / vm;
}

// One launch per resolution r: grid rows * tiles[r]; workgroup b owns slot
// blk0[r] + b.  A kernel per n_fft, so that each carries its own register and
// LDS budget (n_fft = 4096 needs 4 butterflies per thread, n_fft = 64 one).
template <int N, bool BWD>
__global__ __launch_bounds__(kThreads) void loss_frames_kernel(LossParams p, int r) {
    using G = Geo<N>;
    constexpr int H = N / 2;
    __shared__ float re[G::kConc * N];
    __shared__ float im[G::kConc * N];
    __shared__ float red[3 * kWaves];
    // nz[2c], nz[2c + 1]: the value's / the target's frame in slot c has a nonzero
    // sample.  A frame of zeros has the spectrum 0 (|V| = 0: no gradient); read
    // back out of the shared FFT it would be the other signal's rounding noise.
    __shared__ int nz[2 * G::kConc];
    const int local = blockIdx.x;
    float sd = 0.f, st = 0.f, sl = 0.f;
    const float2* tw = reinterpret_cast<const float2*>(p.table[r]);
    const float* win = p.table[r] + 2 * N;
    const int frames = p.frames[r], hop = p.hop[r], wl = p.win[r];
    const int off = (N - wl) / 2;                                 // torch.stft centres the window
    const int row = local / p.tiles[r];
    const int f_tile = (local % p.tiles[r]) * G::kTile;
    const float* vrow = p.value + (int64_t)row * p.t_len;
    const float* trow = p.target + (int64_t)row * p.t_len;
    const bool multires = p.kind == RAVE_STFT_LOSS_MULTIRES;
    float c_lin = 0.f, c_log = 0.f;
    if (BWD) {
        c_lin = p.saved[4 * r + 2] * p.grad_out[0];
        c_log = p.saved[4 * r + 3] * p.grad_out[multires ? 1 : 0];
    }
    float* frow = BWD ? p.frames_ws + p.ws0[r] + (int64_t)row * frames * wl : nullptr;
    for (int pass = 0; pass < G::kPasses; ++pass) {
        const int f0 = f_tile + pass * G::kConc;
        if (f0 >= frames) break;                                  // uniform over the workgroup
        if (threadIdx.x < 2 * G::kConc) nz[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll 4
        for (int u = 0; u < G::kConc * N / kThreads; ++u) {
            const int e = threadIdx.x + u * kThreads;
            const int f = f0 + e / N, j = e % N;
            const int jw = j - off;
            float a = 0.f, b = 0.f;
            if (f < frames && jw >= 0 && jw < wl) {
                const int i = reflect(f * hop + j - H, p.t_len);
                const float w = win[jw];
                a = w * vrow[i];
                b = w * trow[i];
            }
            re[e] = a;
            im[e] = b;
            if (a != 0.f) nz[2 * (e / N)] = 1;                      // every writer stores the same 1
            if (b != 0.f) nz[2 * (e / N) + 1] = 1;
        }
        __syncthreads();
        fft_lds<N>(re, im, tw);
        // Thread (c, k) reads Z[k], Z[N-k] of frame slot c and, backward, rewrites
        // exactly those (k = 0: bins 0 and H), so no barrier separates the two.
#pragma unroll 2
        for (int u = 0; u < G::kConc * H / kThreads; ++u) {
            const int e = threadIdx.x + u * kThreads;
            const int c = e / H, k = e % H;
            if (f0 + c >= frames) continue;
            float* zr = re + c * N;
            float* zi = im + c * N;
            const bool vz = nz[2 * c] == 0, tz = nz[2 * c + 1] == 0;
            if (k == 0) {
                // DC and Nyquist are their own mirror: V = Re Z, T = Im Z
                const float v0 = vz ? 0.f : zr[0], t0 = tz ? 0.f : zi[0];
                const float vh = vz ? 0.f : zr[H], th = tz ? 0.f : zi[H];
                const float g0 = bin_term<BWD>(multires, p.eps, v0 * v0, t0 * t0, c_lin, c_log, sd, st, sl);
                const float gh = bin_term<BWD>(multires, p.eps, vh * vh, th * th, c_lin, c_log, sd, st, sl);
                if (BWD) {
                    zr[0] = g0 * v0;
                    zi[0] = 0.f;
                    zr[H] = gh * vh;
                    zi[H] = 0.f;
                }
            } else {
                const float ar = zr[k], ai = zi[k], br = zr[N - k], bi = zi[N - k];
                const float vre = vz ? 0.f : 0.5f * (ar + br), vim = vz ? 0.f : 0.5f * (ai - bi);   // V[k]
                const float tre = tz ? 0.f : 0.5f * (ai + bi), tim = tz ? 0.f : 0.5f * (br - ar);   // T[k]
                const float g = bin_term<BWD>(multires, p.eps, vre * vre + vim * vim, tre * tre + tim * tim, c_lin,
                                              c_log, sd, st, sl);
                if (BWD) {
                    zr[k] = g * vre;                              // conj G
                    zi[k] = -(g * vim);
                    zr[N - k] = 0.f;
                    zi[N - k] = 0.f;
                }
            }
        }
        __syncthreads();
        if (BWD) {
            fft_lds<N>(re, im, tw);
#pragma unroll 4
            for (int u = 0; u < G::kConc * N / kThreads; ++u) {
                const int e = threadIdx.x + u * kThreads;
                const int f = f0 + e / N, jw = e % N - off;
                if (f < frames && jw >= 0 && jw < wl) frow[(int64_t)f * wl + jw] = re[e] * win[jw];
            }
            __syncthreads();                                      // the next pass overwrites re / im
        }
    }
    if (BWD) return;
    sd = wave_sum(sd);
    st = wave_sum(st);
    sl = wave_sum(sl);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w] = sd;
        red[kWaves + w] = st;
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
        float* slot = p.slots + ((int64_t)p.blk0[r] + blockIdx.x) * 4;
        slot[0] = a;
        slot[1] = b;
        slot[2] = c;
        slot[3] = 0.f;
    }
}

// One workgroup: per resolution, every thread adds the slots t, t + 256, ... in
// double, then a fixed-order tree over the workgroup.
__global__ __launch_bounds__(kThreads) void loss_finalize_kernel(LossParams p, float* out, float* saved) {
    __shared__ double red[3][kThreads];
    const bool multires = p.kind == RAVE_STFT_LOSS_MULTIRES;
    double t0 = 0.0, t1 = 0.0;
    for (int r = 0; r < p.n_res; ++r) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int i = p.blk0[r] + threadIdx.x; i < p.blk0[r + 1]; i += kThreads) {
            const float* slot = p.slots + (int64_t)i * 4;
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
            const double sdd = red[0][0], stt = red[1][0];
            const double count = (double)p.rows * (double)(p.n[r] / 2 + 1) * (double)p.frames[r];
            const double lg = red[2][0] / count;
            double lin, c_lin, c_log;
            if (multires) {
                lin = sqrt(sdd) / sqrt(stt);
                // d lin / d mag = -(T - V) c_lin; torch's norm has gradient 0 at 0
                c_lin = sdd > 0.0 ? 1.0 / (sqrt(sdd) * sqrt(stt) * (double)p.n_res) : 0.0;
                c_log = 1.0 / (count * (double)p.n_res);
                t0 += lin;
                t1 += lg;
            } else {
                lin = sdd / stt;
                c_lin = 2.0 / stt;
                c_log = 1.0 / count;
                t0 += lin + lg;
            }
            out[2 + 2 * r] = (float)lin;
            out[3 + 2 * r] = (float)lg;
            saved[4 * r] = (float)sdd;
            saved[4 * r + 1] = (float)stt;
            saved[4 * r + 2] = (float)c_lin;
            saved[4 * r + 3] = (float)c_log;
        }
        __syncthreads();                                          // red is reused by the next resolution
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(multires ? t0 / (double)p.n_res : t0);
        out[1] = (float)(multires ? t1 / (double)p.n_res : 0.0);
    }
}

// Overlap-add as a gather: one thread per output sample.  In padded coordinates
// (u = sample index, -n/2 <= u < t_len + n/2) frame f holds u in
// [f hop + a, f hop + a + win), a = (n - win)/2 - n/2; sample t is hit at u = t
// and, through the reflect pads, at u = -t (1 <= t <= n/2) and u = 2 (t_len - 1)
// - t (t_len - 1 - n/2 <= t <= t_len - 2).
__global__ __launch_bounds__(kThreads) void loss_gather_kernel(LossParams p) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)p.rows * p.t_len) return;
    const int row = (int)(idx / p.t_len), t = (int)(idx % p.t_len);
    float acc = 0.f;
    for (int r = 0; r < p.n_res; ++r) {
        const int h = p.n[r] / 2, hop = p.hop[r], wl = p.win[r], frames = p.frames[r];
        const int a = (p.n[r] - wl) / 2 - h;
        const float* frow = p.frames_ws + p.ws0[r] + (int64_t)row * frames * wl;
        for (int img = 0; img < 3; ++img) {
            int u = t;
            if (img == 1) {
                if (t < 1 || t > h) continue;
                u = -t;
            } else if (img == 2) {
                if (t > p.t_len - 2 || t < p.t_len - 1 - h) continue;
                u = 2 * (p.t_len - 1) - t;
            }
            const int d = u - a;                                  // offset from frame 0's first sample
            if (d < 0) continue;
            const int f_hi = min(d / hop, frames - 1);
            const int lo = d - wl + 1;
            const int f_lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
            for (int f = f_lo; f <= f_hi; ++f) acc += frow[(int64_t)f * wl + (d - f * hop)];
        }
    }
    p.grad_value[idx] = acc;
}

// ------------------------------------------------------------------ host
bool geometry_ok(int n, int win) { return scale_supported(n) && win >= 1 && win <= n; }

// Validation shared by the workspace query and the ops (pointers excluded).
int check_loss_shape(const rave_stft_loss_args* a, LossParams* p, int64_t* ws_floats) {
    RAVE_CHECK_ARG(a != nullptr, "stft_loss: null arguments");
    RAVE_CHECK_ARG(a->kind == RAVE_STFT_LOSS_V1 || a->kind == RAVE_STFT_LOSS_MULTIRES,
                   "stft_loss: kind " + std::to_string(a->kind) + " is neither RAVE_STFT_LOSS_V1 nor _MULTIRES");
    RAVE_CHECK_ARG(a->n_res >= 1 && a->n_res <= RAVE_STFT_MAX_SCALES,
                   "stft_loss: 1 to " + std::to_string(RAVE_STFT_MAX_SCALES) + " resolutions per call, got " +
                       std::to_string(a->n_res));
    RAVE_CHECK_ARG(a->rows > 0 && a->t_len > 0, "stft_loss: rows and t_len must be positive");
    RAVE_CHECK_ARG(a->t_len <= (1 << 30), "stft_loss: t_len above 2^30");
    RAVE_CHECK_ARG((int64_t)a->rows * a->t_len < (1LL << 38), "stft_loss: rows * t_len too large for one launch");
    if (a->kind == RAVE_STFT_LOSS_V1)
        RAVE_CHECK_ARG(std::isfinite(a->log_epsilon) && a->log_epsilon > 0.f,
                       "stft_loss: log_epsilon must be positive");
    int64_t blocks = 0, frame_floats = 0;
    for (int r = 0; r < a->n_res; ++r) {
        const int n = a->n_fft[r], hop = a->hop[r], win = a->win[r];
        RAVE_CHECK_ARG(scale_supported(n),
                       "stft_loss: n_fft " + std::to_string(n) + " is not a power of two in [64, 4096]");
        RAVE_CHECK_ARG(win >= 1 && win <= n,
                       "stft_loss: win " + std::to_string(win) + " must be in [1, n_fft = " + std::to_string(n) + "]");
        RAVE_CHECK_ARG(hop >= 1, "stft_loss: hop " + std::to_string(hop) + " must be at least 1");
        RAVE_CHECK_ARG(a->t_len > n / 2, "stft_loss: reflect padding needs t_len > n_fft / 2 (n_fft " +
                                             std::to_string(n) + ", t_len " + std::to_string(a->t_len) + ")");
        const int frames = 1 + a->t_len / hop;
        const int tiles = ceil_div(frames, tile_of(n));
        p->n[r] = n;
        p->hop[r] = hop;
        p->win[r] = win;
        p->frames[r] = frames;
        p->tiles[r] = tiles;
        p->blk0[r] = (int)blocks;
        p->ws0[r] = frame_floats;
        blocks += (int64_t)a->rows * tiles;
        frame_floats += (int64_t)a->rows * frames * win;
        RAVE_CHECK_ARG(blocks < (1LL << 30), "stft_loss: rows * frames too large for one launch");
        RAVE_CHECK_ARG(frame_floats < (1LL << 40), "stft_loss: rows * frames * win too large");
    }
    p->blk0[a->n_res] = (int)blocks;
    p->rows = a->rows;
    p->t_len = a->t_len;
    p->n_res = a->n_res;
    p->kind = a->kind;
    p->eps = a->kind == RAVE_STFT_LOSS_V1 ? a->log_epsilon : 0.f;
    *ws_floats = 4 * blocks + frame_floats;
    return RAVE_OK;
}

// Pointers common to both directions.
int bind_loss(const rave_stft_loss_args* a, LossParams* p) {
    RAVE_CHECK_ARG(a->target && a->value && a->workspace && a->saved,
                   "stft_loss: null target, value, workspace or saved");
    for (int r = 0; r < a->n_res; ++r) {
        RAVE_CHECK_ARG(a->tables[r] != nullptr, "stft_loss: null table for resolution " + std::to_string(r));
        p->table[r] = a->tables[r];
    }
    p->value = a->value;
    p->target = a->target;
    p->slots = a->workspace;
    p->frames_ws = a->workspace + 4 * (int64_t)p->blk0[p->n_res];
    p->saved = a->saved;
    p->grad_out = a->grad_out;
    p->grad_value = a->grad_value;
    return RAVE_OK;
}

template <int N, bool BWD>
void launch_frames_n(const LossParams& p, int r, hipStream_t st) {
    launch(loss_frames_kernel<N, BWD>, dim3(p.blk0[r + 1] - p.blk0[r]), dim3(kThreads), 0, st, p, r);
}

template <bool BWD>
int launch_frames(const LossParams& p, hipStream_t st, const char* what) {
    for (int r = 0; r < p.n_res; ++r) {
        switch (p.n[r]) {
            case 64: launch_frames_n<64, BWD>(p, r, st); break;
            case 128: launch_frames_n<128, BWD>(p, r, st); break;
            case 256: launch_frames_n<256, BWD>(p, r, st); break;
            case 512: launch_frames_n<512, BWD>(p, r, st); break;
            case 1024: launch_frames_n<1024, BWD>(p, r, st); break;
            case 2048: launch_frames_n<2048, BWD>(p, r, st); break;
            default: launch_frames_n<4096, BWD>(p, r, st); break;
        }
        const int rc = launch_status(what);
        if (rc != RAVE_OK) return rc;
    }
    return RAVE_OK;
}

}  // namespace
}  // namespace rave

using namespace rave;

extern "C" int64_t rave_stft_loss_table_size(int n_fft, int win) {
    if (!geometry_ok(n_fft, win)) {
        set_error("stft_loss_table_size: n_fft " + std::to_string(n_fft) + " must be a power of two in [64, 4096] and win " +
                  std::to_string(win) + " in [1, n_fft]");
        return -1;
    }
    return 2 * (int64_t)n_fft + win;
}

extern "C" int rave_stft_loss_pack_table(int n_fft, int win, float* out) {
    RAVE_CHECK_ARG(geometry_ok(n_fft, win), "stft_loss_pack_table: n_fft " + std::to_string(n_fft) +
                                                " must be a power of two in [64, 4096] and win " + std::to_string(win) +
                                                " in [1, n_fft]");
    RAVE_CHECK_ARG(out != nullptr, "stft_loss_pack_table: null output");
    const double pi2 = 2.0 * 3.14159265358979323846;
    for (int k = 0; k < n_fft; ++k) {
        out[2 * k] = (float)std::cos(pi2 / (double)n_fft * k);
        out[2 * k + 1] = (float)(-std::sin(pi2 / (double)n_fft * k));
    }
    for (int i = 0; i < win; ++i) out[2 * n_fft + i] = (float)(0.5 - 0.5 * std::cos(pi2 / (double)win * i));
    return RAVE_OK;
}

extern "C" int64_t rave_stft_loss_workspace(const rave_stft_loss_args* a) {
    LossParams p;
    int64_t floats = 0;
    if (check_loss_shape(a, &p, &floats) != RAVE_OK) return -1;
    return floats * (int64_t)sizeof(float);
}

extern "C" int rave_stft_loss_forward(const rave_stft_loss_args* a, void* stream) {
    LossParams p;
    int64_t floats = 0;
    int rc = check_loss_shape(a, &p, &floats);
    if (rc != RAVE_OK) return rc;
    rc = bind_loss(a, &p);
    if (rc != RAVE_OK) return rc;
    RAVE_CHECK_ARG(a->out != nullptr, "stft_loss_forward: null out");
    hipStream_t st = as_stream(stream);
    rc = launch_frames<false>(p, st, "stft_loss_forward");
    if (rc != RAVE_OK) return rc;
    launch(loss_finalize_kernel, dim3(1), dim3(kThreads), 0, st, p, a->out, a->saved);
    return launch_status("stft_loss_forward finalize");
}

extern "C" int rave_stft_loss_backward(const rave_stft_loss_args* a, void* stream) {
    LossParams p;
    int64_t floats = 0;
    int rc = check_loss_shape(a, &p, &floats);
    if (rc != RAVE_OK) return rc;
    rc = bind_loss(a, &p);
    if (rc != RAVE_OK) return rc;
    RAVE_CHECK_ARG(a->grad_out && a->grad_value, "stft_loss_backward: null grad_out or grad_value");
    hipStream_t st = as_stream(stream);
    rc = launch_frames<true>(p, st, "stft_loss_backward");
    if (rc != RAVE_OK) return rc;
    const int64_t samples = (int64_t)p.rows * p.t_len;
    launch(loss_gather_kernel, dim3((uint32_t)ceil_div64(samples, kThreads)), dim3(kThreads), 0, st, p);
    return launch_status("stft_loss_backward gather");
}
