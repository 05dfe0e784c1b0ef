// YIN pitch tracking and the f0 one-hot conditioning (rave/pitch_utils.py:
// estimate and its helpers :15-86, get_pitch :90-96, one_hot / get_f0_norm in
// 'abs' mode :98-127; the 257 channels ScriptedRAVE.myforward concatenates after
// the latent and the speaker embedding, scripts/export.py:358-397).
//
// One group of threads owns one frame: the whole workgroup (256 threads) when
// tau_max > 256, one wave otherwise (four frames per workgroup).  The frame sits
// in LDS as fp32; everything derived from it is double.  The reference takes the
// autocorrelation by FFT; here it is the direct sum: a product of two fp32
// values is exact in double, CDNA4's vector FP64 FMA peak is half its packed
// fp32 peak, and the sum is 0.6 M multiply-adds per frame at the get_pitch
// binding, so double is affordable: r(tau), the
// prefix sums and the cmdf carry double rounding only and the period search
// makes the float64 reference's decisions.  A thread owns four consecutive lags
// and walks the frame four samples a step: one broadcast ds_read_b128 and one
// new ds_read_b128 feed sixteen fused multiply-adds.
//
// d(tau) overwrites sq[tau] and cmdf[i] overwrites d(i + 1), each slot read only
// by the thread that rewrites it (sq[L - tau] lies above tau_max), so a frame
// costs 12 L bytes of LDS.  No atomics: reruns are bitwise identical.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"

namespace rave {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxL = 4410;              // estimate()'s own default: 20 Hz at 44.1 kHz
constexpr int kWaveTauMax = 256;         // one wave per frame up to this tau_max (4 lags per lane)
constexpr int kMaxBins = 4096;

struct PitchParams {
    const float* x;
    float* f0;                           // may be null (fused call that keeps only the one-hot)
    float* cmdf;                         // may be null
    float* y;                            // may be null (rave_yin)
    int64_t y_sb, y_sc;
    double threshold;
    int rows, t_len, frames, total;      // total = rows * frames
    int tau_min, tau_max, len, stride;   // len = 2 tau_max
    int xpad;                            // floats of a group's frame in LDS (zero tail included)
    int group_bytes;                     // LDS bytes per group
    int bins;
    float sr, log_lo, log_span;
};

// get_f0_norm, 'abs' mode, with the reference's arithmetic as written: class of
// v = (log f0 - log 40) / log(400 - log 40) + 0.5 among linspace(0, 1, bins + 1)
// (bucketize(right=True) - 1).  bins is a power of two, so the edges are exact
// and the class is floor(v bins).  Class `bins` catches f0 = 0 (log of NaN),
// v < 0 (index -1 wraps) and v >= 1.
__device__ __forceinline__ int f0_class(float f0, float log_lo, float log_span, int bins) {
    if (f0 == 0.f) return bins;
    const float v = (logf(f0) - log_lo) / log_span + 0.5f;
    if (!(v >= 0.f) || !(v < 1.f)) return bins;
    return (int)floorf(v * (float)bins);
}

// Exclusive prefix sum over the TPF threads of a group.  wtot: kWaves doubles.
template <int TPF>
__device__ __forceinline__ double group_scan(double v, double* wtot) {
    const int lane = threadIdx.x & 63;
    double inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double n = __shfl_up(inc, o, 64);
        if (lane >= o) inc += n;
    }
    double ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.0;
    if (TPF > 64) {
        const int wave = threadIdx.x >> 6;
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        double base = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
            if (w < wave) base += wtot[w];
        __syncthreads();                                          // wtot is reused by the next scan
        ex += base;
    }
    return ex;
}

template <int TPF>
__device__ __forceinline__ int group_min(int v, int* wmin) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if (TPF > 64) {
        if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = v;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v = min(v, wmin[w]);
        __syncthreads();
    }
    return v;
}

template <int TPF>
__global__ __launch_bounds__(kThreads) void yin_kernel(PitchParams p) {
    extern __shared__ __align__(16) double lds[];
    __shared__ double wtot[kWaves];
    __shared__ int wmin[kWaves];
    constexpr int kGroups = kThreads / TPF;
    const int g = threadIdx.x / TPF, t = threadIdx.x % TPF;
    const int frame = blockIdx.x * kGroups + g;                   // over (row, frame)
    const bool live = frame < p.total;
    const int row = live ? frame / p.frames : 0, f = live ? frame % p.frames : 0;
    const int L = p.len, tau_max = p.tau_max;

    char* base = reinterpret_cast<char*>(lds) + (size_t)g * p.group_bytes;
    double* sq = reinterpret_cast<double*>(base);                 // L + 1 prefix sums; then d, then cmdf
    float* xs = reinterpret_cast<float*>(base + p.group_bytes - (size_t)p.xpad * sizeof(float));

    // the frame, zero beyond the signal (a signal shorter than L is one padded
    // frame) and beyond L (the lag loop reads up to 7 past its last sample)
    const float* xr = p.x + (int64_t)row * p.t_len + (int64_t)f * p.stride;
    const int avail = live ? min(L, p.t_len - f * p.stride) : 0;
    for (int i = t; i < p.xpad; i += TPF) xs[i] = i < avail ? xr[i] : 0.f;
    __syncthreads();

    // sq[i] = sum_{j < i} x_j^2
    {
        const int chunk = ceil_div(L, TPF);
        const int lo = min(L, t * chunk), hi = min(L, lo + chunk);
        double s = 0.0;
        for (int i = lo; i < hi; ++i) s += (double)xs[i] * (double)xs[i];
        double run = group_scan<TPF>(s, wtot);
        if (t == 0) sq[0] = 0.0;
        for (int i = lo; i < hi; ++i) {
            run += (double)xs[i] * (double)xs[i];
            sq[i + 1] = run;
        }
    }
    __syncthreads();

    // d(tau) = c0 + (sq[L - tau] - sq[tau]) - 2 r(tau), r(tau) = sum_j x_j x_{j + tau}
    // over j + tau < L: the zero tail ends the sum for every lag of the tile
    const double c0 = sq[L];
    const float4* x4 = reinterpret_cast<const float4*>(xs);
    for (int t0 = 4 * t; t0 < tau_max; t0 += 4 * TPF) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        float4 b0 = x4[t0 >> 2];
        for (int j = 0; j + t0 < L; j += 4) {
            const float4 a = x4[j >> 2];
            const float4 b1 = x4[((j + t0) >> 2) + 1];
            const double av[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
            const double bv[7] = {(double)b0.x, (double)b0.y, (double)b0.z, (double)b0.w,
                                  (double)b1.x, (double)b1.y, (double)b1.z};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = fma(av[i], bv[i + c], acc[c]);
            b0 = b1;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int tau = t0 + c;
            if (tau < tau_max) sq[tau] = (c0 + (sq[L - tau] - sq[tau])) - 2.0 * acc[c];
        }
    }
    __syncthreads();

    // cmdf[i] = d(i + 1) (i + 1) / max(sum_{k <= i} d(k + 1), 1e-5), i < tau_max - 1,
    // kept at sq[i + 1]; the slice [tau_min:] goes out in fp32 when asked for
    const int m = tau_max - 1 - p.tau_min;
    {
        const int n = tau_max - 1;
        const int chunk = ceil_div(n, TPF);
        const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
        double s = 0.0;
        for (int i = lo; i < hi; ++i) s += sq[i + 1];
        double run = group_scan<TPF>(s, wtot);
        float* co = (p.cmdf && live) ? p.cmdf + (int64_t)frame * m : nullptr;
        for (int i = lo; i < hi; ++i) {
            const double d = sq[i + 1];
            run += d;
            const double v = d * (double)(i + 1) / (run < 1e-5 ? 1e-5 : run);
            sq[i + 1] = v;
            if (co && i >= p.tau_min) co[i - p.tau_min] = (float)v;
        }
    }
    __syncthreads();

    // _search: first index below the threshold (index 0 or none: unvoiced), then
    // the first index at or beyond it where the cmdf stops falling (the last
    // index counts as rising)
    const double* cm = sq + p.tau_min + 1;
    int fb = INT_MAX;
    for (int j = t; j < m; j += TPF)
        if (cm[j] < p.threshold) {
            fb = j;
            break;
        }
    fb = group_min<TPF>(fb, wmin);
    int idx = INT_MAX;
    if (fb > 0 && fb != INT_MAX)
        for (int j = fb + t; j < m; j += TPF)
            if (j == m - 1 || cm[j + 1] - cm[j] >= 0.0) {
                idx = j;
                break;
            }
    idx = group_min<TPF>(idx, wmin);
    if (idx == INT_MAX) idx = 0;
    const float f0 = idx > 0 ? p.sr / (float)(idx + p.tau_min + 1) : 0.f;
    if (!live) return;
    if (p.f0 && t == 0) p.f0[frame] = f0;
    if (p.y) {
        const int cls = f0_class(f0, p.log_lo, p.log_span, p.bins);
        float* yc = p.y + (int64_t)row * p.y_sb + f;
        for (int c = t; c <= p.bins; c += TPF) yc[(int64_t)c * p.y_sc] = c == cls ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void f0_onehot_kernel(rave_f0_onehot_args a) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t per_b = (int64_t)(a.bins + 1) * a.frames;
    if (e >= per_b * a.batch) return;
    const int b = (int)(e / per_b);
    const int c = (int)((e % per_b) / a.frames), t = (int)(e % a.frames);
    const int cls = f0_class(a.f0[(int64_t)b * a.frames + t], a.log_lo, a.log_span, a.bins);
    a.y[(int64_t)b * a.y_sb + (int64_t)c * a.y_sc + t] = c == cls ? 1.f : 0.f;
}

// ------------------------------------------------------------------ host
// estimate()'s host arithmetic, in its order; pointers excluded.
int check_yin(const rave_yin_args* a, PitchParams* p, const char* op) {
    const std::string who = std::string(op) + ": ";
    RAVE_CHECK_ARG(a != nullptr, who + "null arguments");
    RAVE_CHECK_ARG(a->rows > 0 && a->t_len > 0, who + "rows and t_len must be positive");
    RAVE_CHECK_ARG(a->t_len <= (1 << 30), who + "t_len above 2^30");
    RAVE_CHECK_ARG(a->sample_rate > 0, who + "sample_rate must be positive");
    RAVE_CHECK_ARG(std::isfinite(a->pitch_min) && std::isfinite(a->pitch_max) && a->pitch_min > 0.0,
                   who + "pitch_min and pitch_max must be finite and positive");
    RAVE_CHECK_ARG(a->pitch_max > a->pitch_min, who + "pitch_max must exceed pitch_min");
    RAVE_CHECK_ARG(!std::isnan(a->threshold), who + "threshold is NaN");
    const double sr = (double)a->sample_rate;
    if (sr / a->pitch_min > (double)(kMaxL / 2 + 1)) {
        set_error(who + "frame length 2 int(sample_rate / pitch_min) exceeds " + std::to_string(kMaxL));
        return RAVE_ERR_UNSUPPORTED;
    }
    const int tau_min = (int)(sr / a->pitch_max);
    const int tau_max = (int)(sr / a->pitch_min);
    if (2 * tau_max > kMaxL) {
        set_error(who + "frame length " + std::to_string(2 * tau_max) + " exceeds " + std::to_string(kMaxL));
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(tau_min < tau_max - 1, who + "no lag left to search: tau_min " + std::to_string(tau_min) +
                                              " >= tau_max - 1 = " + std::to_string(tau_max - 1));
    const double fs = a->frame_stride * sr;
    RAVE_CHECK_ARG(std::isfinite(fs) && fs < 2147483647.0, who + "frame_stride out of range");
    const int stride = (int)fs;
    RAVE_CHECK_ARG(stride >= 1, who + "frame_stride is below one sample (stride 0)");
    const int L = 2 * tau_max;
    const int frames = a->t_len < L ? 1 : (a->t_len - L) / stride + 1;
    RAVE_CHECK_ARG((int64_t)a->rows * frames < (1LL << 30), who + "rows * frames too large for one launch");
    std::memset(p, 0, sizeof(*p));
    p->threshold = a->threshold;
    p->rows = a->rows;
    p->t_len = a->t_len;
    p->frames = frames;
    p->total = a->rows * frames;
    p->tau_min = tau_min;
    p->tau_max = tau_max;
    p->len = L;
    p->stride = stride;
    p->xpad = (L + 3) / 4 * 4 + 8;
    p->group_bytes = ((L + 1) * (int)sizeof(double) + 15) / 16 * 16 + p->xpad * (int)sizeof(float);
    p->sr = (float)a->sample_rate;
    return RAVE_OK;
}

int check_yin_pointers(const rave_yin_args* a, bool need_f0, const char* op) {
    const std::string who = std::string(op) + ": ";
    RAVE_CHECK_ARG(a->x != nullptr, who + "null x");
    RAVE_CHECK_ARG(!need_f0 || a->f0 != nullptr, who + "null f0");
    RAVE_CHECK_ARG(a->x_sr == (int64_t)a->t_len, who + "rows of x must be contiguous (x_sr == t_len)");
    return RAVE_OK;
}

int check_onehot(const rave_f0_onehot_args* a, bool need_f0, const char* op) {
    const std::string who = std::string(op) + ": ";
    RAVE_CHECK_ARG(a != nullptr, who + "null one-hot arguments");
    RAVE_CHECK_ARG(a->batch > 0 && a->frames > 0, who + "batch and frames must be positive");
    if (a->bins < 1 || a->bins > kMaxBins || (a->bins & (a->bins - 1)) != 0) {
        set_error(who + "bins must be a power of two in [1, " + std::to_string(kMaxBins) + "], got " +
                  std::to_string(a->bins));
        return RAVE_ERR_UNSUPPORTED;
    }
    RAVE_CHECK_ARG(std::isfinite(a->log_lo) && std::isfinite(a->log_span) && a->log_span != 0.f,
                   who + "log_lo / log_span must be finite, log_span non-zero");
    RAVE_CHECK_ARG(a->y_sc >= a->frames, who + "y_sc below frames");
    RAVE_CHECK_ARG(a->batch == 1 || a->y_sb >= (int64_t)a->bins * a->y_sc + a->frames, who + "y_sb overlaps batches");
    RAVE_CHECK_ARG((int64_t)a->batch * (a->bins + 1) * a->frames < (1LL << 38), who + "output too large for one launch");
    RAVE_CHECK_ARG(a->y != nullptr, who + "null y");
    RAVE_CHECK_ARG(!need_f0 || a->f0 != nullptr, who + "null f0");
    return RAVE_OK;
}

int launch_yin(PitchParams& p, hipStream_t st, const char* op) {
    if (p.tau_max <= kWaveTauMax) {
        constexpr int kGroups = kThreads / 64;
        launch(yin_kernel<64>, dim3(ceil_div(p.total, kGroups)), dim3(kThreads), (uint32_t)(kGroups * p.group_bytes),
               st, p);
    } else {
        launch(yin_kernel<kThreads>, dim3(p.total), dim3(kThreads), (uint32_t)p.group_bytes, st, p);
    }
    return launch_status(op);
}

}  // namespace
}  // namespace rave

using namespace rave;

extern "C" int rave_yin_shape(const rave_yin_args* a, int32_t* out) {
    PitchParams p;
    const int rc = check_yin(a, &p, "yin_shape");
    if (rc != RAVE_OK) return rc;
    RAVE_CHECK_ARG(out != nullptr, "yin_shape: null output");
    out[0] = p.tau_min;
    out[1] = p.tau_max;
    out[2] = p.len;
    out[3] = p.stride;
    out[4] = p.frames;
    return RAVE_OK;
}

extern "C" int rave_yin(const rave_yin_args* a, void* stream) {
    PitchParams p;
    int rc = check_yin(a, &p, "yin");
    if (rc != RAVE_OK) return rc;
    rc = check_yin_pointers(a, true, "yin");
    if (rc != RAVE_OK) return rc;
    p.x = a->x;
    p.f0 = a->f0;
    p.cmdf = a->cmdf;
    return launch_yin(p, as_stream(stream), "yin");
}

extern "C" int rave_f0_onehot(const rave_f0_onehot_args* a, void* stream) {
    const int rc = check_onehot(a, true, "f0_onehot");
    if (rc != RAVE_OK) return rc;
    const int64_t total = (int64_t)a->batch * (a->bins + 1) * a->frames;
    launch(f0_onehot_kernel, dim3((uint32_t)ceil_div64(total, kThreads)), dim3(kThreads), 0, as_stream(stream), *a);
    return launch_status("f0_onehot");
}

extern "C" int rave_pitch_onehot(const rave_yin_args* a, const rave_f0_onehot_args* h, void* stream) {
    PitchParams p;
    int rc = check_yin(a, &p, "pitch_onehot");
    if (rc != RAVE_OK) return rc;
    rc = check_yin_pointers(a, false, "pitch_onehot");
    if (rc != RAVE_OK) return rc;
    rc = check_onehot(h, false, "pitch_onehot");
    if (rc != RAVE_OK) return rc;
    RAVE_CHECK_ARG(h->batch == a->rows && h->frames == p.frames,
                   "pitch_onehot: one-hot is (" + std::to_string(h->batch) + ", " + std::to_string(h->frames) +
                       "), the contour (" + std::to_string(a->rows) + ", " + std::to_string(p.frames) + ")");
    p.x = a->x;
    p.f0 = a->f0;
    p.cmdf = a->cmdf;
    p.y = h->y;
    p.y_sb = h->y_sb;
    p.y_sc = h->y_sc;
    p.bins = h->bins;
    p.log_lo = h->log_lo;
    p.log_span = h->log_span;
    return launch_yin(p, as_stream(stream), "pitch_onehot");
}
