// TorchScript binding of the model engine (TORCH_LIBRARY): the operator seam
// nn~ needs.  nn~ (a C++ Max/PD external) loads a TorchScript module and calls
// its registered methods (scripts/export.py:58-480, export_to_ts :618); ctypes
// cannot be scripted, so the engine is exposed as the custom class
// torch.classes.rave_amd.Engine whose methods take and return tensors on
// torch's current HIP stream, and which pickles (def_pickle) so a scripted
// module holding one can be saved and loaded like any .ts file.
//
// Only tensors, ints and strings cross this file; every launch goes through
// the C-ABI (include/rave_amd.h rave_model_* / rave_stream_*).
#include <torch/csrc/autograd/custom_function.h>
#include <torch/custom_class.h>
#include <torch/script.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/rave_amd.h"

namespace {

void check(int rc, const char* what) {
    if (rc == RAVE_OK) return;
    const std::string msg = std::string(what) + ": " + rave_last_error();
    if (rc == RAVE_ERR_ARG) TORCH_CHECK_VALUE(false, msg);
    if (rc == RAVE_ERR_UNSUPPORTED) TORCH_CHECK_NOT_IMPLEMENTED(false, msg);
    TORCH_CHECK(false, msg, " (status ", rc, ")");
}

// rave_model_config <-> a flat int list (the TorchScript-visible form) + leaky slope
// n_band .. n_ratios (7), ratios, n_dilations, dilations, am / causal / act / adain (4),
// biases (2), noise / hidden / bands / n_noise_ratios (4), noise_ratios, rvq x2 + fuse (3)
constexpr int kCfgInts = 7 + 2 * RAVE_MAX_RATIOS + RAVE_MAX_RATIOS * RAVE_MAX_DILATIONS + 4 + 2 + 4 +
                         RAVE_MAX_RATIOS + 3;

rave_model_config config_from(const std::vector<int64_t>& v, double slope) {
    TORCH_CHECK_VALUE((int)v.size() == kCfgInts, "engine config: expected ", kCfgInts, " ints, got ", v.size());
    rave_model_config c{};
    size_t i = 0;
    auto nx = [&]() { return (int32_t)v[i++]; };
    c.n_band = nx(); c.enc_bands = nx(); c.capacity = nx(); c.latent_size = nx();
    c.kernel_size = nx(); c.speaker_size = nx(); c.n_ratios = nx();
    for (int k = 0; k < RAVE_MAX_RATIOS; ++k) c.ratios[k] = nx();
    for (int k = 0; k < RAVE_MAX_RATIOS; ++k) c.n_dilations[k] = nx();
    for (int k = 0; k < RAVE_MAX_RATIOS; ++k)
        for (int j = 0; j < RAVE_MAX_DILATIONS; ++j) c.dilations[k][j] = nx();
    c.amplitude_modulation = nx(); c.causal = nx(); c.activation = nx(); c.adain = nx();
    c.conv_bias = nx(); c.convt_bias = nx();
    c.noise = nx(); c.noise_hidden = nx(); c.noise_bands = nx(); c.n_noise_ratios = nx();
    for (int k = 0; k < RAVE_MAX_RATIOS; ++k) c.noise_ratios[k] = nx();
    c.rvq_quantizers = nx(); c.rvq_codebook_size = nx(); c.fuse_units = nx();
    c.leaky_slope = (float)slope;
    return c;
}

struct Engine : torch::CustomClassHolder {
    // constructor arguments, kept for pickling
    std::vector<int64_t> cfg_ints;
    double slope;
    std::vector<std::string> names;
    std::vector<at::Tensor> params;
    at::Tensor speaker;
    int64_t precision;
    int64_t stream_block;
    // engine state
    rave_model_config cfg{};
    rave_model* m = nullptr;
    rave_stream* s_enc = nullptr;   // streaming: one state per direction (nn~'s encode / decode
    rave_stream* s_dec = nullptr;   // methods run independently), created on first use
    int64_t s_enc_b = 0, s_dec_b = 0;
    int device = 0;
    int hop = 1;

    Engine(std::vector<int64_t> ci, double sl, std::vector<std::string> nm, std::vector<at::Tensor> ps, at::Tensor spk,
           int64_t prec, int64_t block)
        : cfg_ints(std::move(ci)), slope(sl), names(std::move(nm)), params(std::move(ps)), speaker(std::move(spk)),
          precision(prec), stream_block(block) {
        TORCH_CHECK_VALUE(names.size() == params.size(), "one tensor per parameter name");
        cfg = config_from(cfg_ints, slope);
        hop = cfg.n_band;
        for (int i = 0; i < cfg.n_ratios; ++i) hop *= cfg.ratios[i];
        std::vector<at::Tensor> host;
        std::vector<rave_param> p(names.size());
        for (size_t i = 0; i < names.size(); ++i) {
            host.push_back(params[i].detach().to(at::kCPU, at::kFloat).contiguous());
            p[i] = rave_param{names[i].c_str(), host.back().data_ptr<float>(), host.back().numel()};
        }
        at::Tensor spk_h = speaker.detach().to(at::kCPU, at::kFloat).contiguous();
        device = c10::hip::current_device();
        check(rave_model_create(&cfg, p.data(), (int)p.size(), spk_h.data_ptr<float>(), (int)precision, &m),
              "rave_model_create");
    }
    ~Engine() override {
        if (s_enc) rave_stream_destroy(s_enc);
        if (s_dec) rave_stream_destroy(s_dec);
        if (m) rave_model_destroy(m);
    }

    void* cur() const { return c10::hip::getCurrentHIPStream(device).stream(); }
    void on_device(const at::Tensor& t, const char* what) const {
        TORCH_CHECK_VALUE(t.is_cuda() && t.get_device() == device, what, " must be on cuda:", device);
    }
    int64_t zc() const { return cfg.latent_size + cfg.speaker_size; }

    at::Tensor encode(at::Tensor x) {
        on_device(x, "x");
        TORCH_CHECK_VALUE(x.dim() == 3 && x.size(1) == 1 && x.scalar_type() == at::kFloat, "x must be (B, 1, T) float32");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        x = x.contiguous();
        auto z = at::empty({x.size(0), zc(), x.size(2) / hop}, x.options());
        check(rave_model_encode(m, x.data_ptr<float>(), (int)x.size(0), (int)x.size(2), z.data_ptr<float>(), cur()),
              "encode");
        return z;
    }
    at::Tensor decode(at::Tensor z) {
        on_device(z, "z");
        TORCH_CHECK_VALUE(z.dim() == 3 && z.size(1) == zc() && z.scalar_type() == at::kFloat,
                          "z must be (B, latent + speaker, F) float32");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        z = z.contiguous();
        auto y = at::empty({z.size(0), 1, z.size(2) * hop}, z.options());
        check(rave_model_decode(m, z.data_ptr<float>(), (int)z.size(0), (int)z.size(2), y.data_ptr<float>(), nullptr,
                                cur()),
              "decode");
        return y;
    }
    at::Tensor forward(at::Tensor x) {
        on_device(x, "x");
        TORCH_CHECK_VALUE(x.dim() == 3 && x.size(1) == 1 && x.scalar_type() == at::kFloat, "x must be (B, 1, T) float32");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        x = x.contiguous();
        auto y = at::empty_like(x);
        check(rave_model_forward(m, x.data_ptr<float>(), (int)x.size(0), (int)x.size(2), y.data_ptr<float>(), nullptr,
                                 cur()),
              "forward");
        return y;
    }
    at::Tensor encode_codes(at::Tensor x) {
        on_device(x, "x");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        x = x.contiguous();
        auto idx = at::empty({x.size(0), (int64_t)cfg.rvq_quantizers, x.size(2) / hop}, x.options().dtype(at::kLong));
        check(rave_model_encode_codes(m, x.data_ptr<float>(), (int)x.size(0), (int)x.size(2), idx.data_ptr<int64_t>(),
                                      cur()),
              "encode_codes");
        return idx;
    }
    at::Tensor decode_codes(at::Tensor idx) {
        on_device(idx, "idx");
        TORCH_CHECK_VALUE(idx.scalar_type() == at::kLong, "idx must be int64");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        idx = idx.contiguous();
        auto y = at::empty({idx.size(0), 1, idx.size(2) * hop}, idx.options().dtype(at::kFloat));
        check(rave_model_decode_codes(m, idx.data_ptr<int64_t>(), (int)idx.size(0), (int)idx.size(2),
                                      y.data_ptr<float>(), nullptr, cur()),
              "decode_codes");
        return y;
    }
    // cached_conv streaming (one block of stream_block samples per call)
    // (one stream object per direction, each built for that direction only)
    rave_stream* stream_for(rave_stream*& s, int64_t& sb, int64_t batch, int direction) {
        if (!s || sb != batch) {
            if (s) rave_stream_destroy(s);
            s = nullptr;
            check(rave_stream_create(m, (int)batch, (int)stream_block, RAVE_STREAM_GRAPH | direction, &s),
                  "rave_stream_create");
            sb = batch;
        }
        return s;
    }
    at::Tensor stream_encode(at::Tensor x) {
        on_device(x, "x");
        TORCH_CHECK_VALUE(x.dim() == 3 && x.size(1) == 1 && x.size(2) == stream_block, "x must be (B, 1, block)");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        x = x.contiguous();
        rave_stream* s = stream_for(s_enc, s_enc_b, x.size(0), RAVE_STREAM_ENCODE_ONLY);
        auto z = at::empty({x.size(0), zc(), stream_block / hop}, x.options());
        check(rave_stream_encode(s, x.data_ptr<float>(), z.data_ptr<float>(), cur()), "stream_encode");
        return z;
    }
    at::Tensor stream_decode(at::Tensor z) {
        on_device(z, "z");
        TORCH_CHECK_VALUE(z.dim() == 3 && z.size(1) == zc() && z.size(2) == stream_block / hop,
                          "z must be (B, latent + speaker, block / hop)");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        z = z.contiguous();
        rave_stream* s = stream_for(s_dec, s_dec_b, z.size(0), RAVE_STREAM_DECODE_ONLY);
        auto y = at::empty({z.size(0), 1, stream_block}, z.options());
        check(rave_stream_decode(s, z.data_ptr<float>(), y.data_ptr<float>(), nullptr, cur()), "stream_decode");
        return y;
    }
    // discrete configs: one block of RVQ indices (B, n_q, block / hop) int64
    at::Tensor stream_encode_codes(at::Tensor x) {
        on_device(x, "x");
        TORCH_CHECK_VALUE(x.dim() == 3 && x.size(1) == 1 && x.size(2) == stream_block, "x must be (B, 1, block)");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        x = x.contiguous();
        rave_stream* s = stream_for(s_enc, s_enc_b, x.size(0), RAVE_STREAM_ENCODE_ONLY);
        auto idx = at::empty({x.size(0), (int64_t)cfg.rvq_quantizers, stream_block / hop}, x.options().dtype(at::kLong));
        check(rave_stream_encode_codes(s, x.data_ptr<float>(), idx.data_ptr<int64_t>(), cur()), "stream_encode_codes");
        return idx;
    }
    at::Tensor stream_decode_codes(at::Tensor idx) {
        on_device(idx, "idx");
        TORCH_CHECK_VALUE(idx.dim() == 3 && idx.size(1) == cfg.rvq_quantizers && idx.size(2) == stream_block / hop &&
                              idx.scalar_type() == at::kLong,
                          "idx must be (B, n_q, block / hop) int64");
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        idx = idx.contiguous();
        rave_stream* s = stream_for(s_dec, s_dec_b, idx.size(0), RAVE_STREAM_DECODE_ONLY);
        auto y = at::empty({idx.size(0), 1, stream_block}, idx.options().dtype(at::kFloat));
        check(rave_stream_decode_codes(s, idx.data_ptr<int64_t>(), y.data_ptr<float>(), nullptr, cur()),
              "stream_decode_codes");
        return y;
    }
    void stream_reset() {
        if (s_enc) check(rave_stream_reset(s_enc, cur()), "stream_reset");
        if (s_dec) check(rave_stream_reset(s_dec, cur()), "stream_reset");
    }
    // AdaIN controls (ScriptedRAVE.update_adain): -1 keeps a flag
    void adain_control(int64_t learn_x, int64_t learn_y, bool reset_x, bool reset_y) {
        check(rave_model_adain_control(m, (int)learn_x, (int)learn_y, reset_x, reset_y, cur()), "adain_control");
    }
    // the constant speaker embedding encode concatenates (nn~ `speaker` choice)
    // 2-D (R, speaker_size): per-row mode, batch row b reads row b (rave_model_set_speakers
    // at row 0).  The table is run-time state: the pickle keeps the shared vector.
    void set_speaker(at::Tensor emb) {
        c10::hip::HIPGuard g((c10::DeviceIndex)device);
        if (emb.dim() == 2) {
            TORCH_CHECK_VALUE(emb.size(0) > 0 && emb.size(1) == cfg.speaker_size, "speaker embeddings must be (R, ",
                              cfg.speaker_size, ")");
            at::Tensor rows = emb.detach().to(at::Device(at::kCUDA, device), at::kFloat).contiguous();
            check(rave_model_set_speakers(m, rows.data_ptr<float>(), (int)rows.size(0), 0, cur()), "set_speakers");
            return;
        }
        TORCH_CHECK_VALUE(emb.numel() == cfg.speaker_size, "speaker embedding must have ", cfg.speaker_size, " values");
        at::Tensor src = emb.detach().to(at::Device(at::kCUDA, device), at::kFloat).contiguous();
        check(rave_model_set_speaker(m, src.data_ptr<float>(), cur()), "set_speaker");
        // src came from torch's caching allocator on this stream, so freeing it on
        // return is stream-ordered after the copy
        speaker = emb.detach().cpu().to(at::kFloat).reshape({-1}).clone();    // travels with the pickle
    }
    // cooperative-unit give-ups of the calls queued so far (rave_model_check; waits for
    // the current stream); encode / decode / stream calls also raise them on entry
    void check_status() { check(rave_model_check(m, 1, cur()), "check"); }
    // launch choices (RAVE.tuning() text: "key value ms" per line), e.g. a pinned plan
    void set_tuning(const std::string& text) { check(rave_model_tuning_set(m, text.c_str()), "tuning_set"); }
    int64_t get_hop() const { return hop; }
    int64_t latent_channels() const { return zc(); }
    int64_t block() const { return stream_block; }
};

// rave_amd::fir -- the Resampler's cached_conv Conv1d (rave/resampler.py:29-58) on
// rave_fir: x (B, T) at any stride; h (P, K); y (B, P * T_out) interleaved.
// Offline: zero padding (pad_left, pad_right).  Streaming: `hist` (B, H) with
// H = pad_left + pad_right + stride_delay is the cached input (CachedConv1d),
// updated in place; T must be a multiple of the stride.
at::Tensor fir_op(at::Tensor x, at::Tensor h, int64_t stride, int64_t pad_left, int64_t pad_right,
                  c10::optional<at::Tensor> hist) {
    TORCH_CHECK_VALUE(x.is_cuda() && x.dim() == 2 && x.scalar_type() == at::kFloat, "x must be (B, T) float32 on GPU");
    TORCH_CHECK_VALUE(h.dim() == 2 && h.scalar_type() == at::kFloat, "h must be (phases, taps) float32");
    TORCH_CHECK_VALUE(stride > 0 && pad_left >= 0 && pad_right >= 0, "bad stride / padding");
    c10::hip::HIPGuard g((c10::DeviceIndex)x.get_device());
    const int64_t B = x.size(0), T = x.size(1), P = h.size(0), K = h.size(1);
    at::Tensor hd = h.to(x.device()).contiguous();
    at::Tensor src;
    int64_t t_in, t_out, pl;
    if (hist.has_value()) {
        at::Tensor hs = *hist;
        TORCH_CHECK_VALUE(hs.is_cuda() && hs.dim() == 2 && hs.size(0) == B && hs.scalar_type() == at::kFloat,
                          "hist must be (B, H) float32 on the GPU");
        TORCH_CHECK_VALUE(T % stride == 0, "streaming block must be a multiple of the stride");
        src = at::cat({hs, x}, 1).contiguous();
        t_in = src.size(1);
        t_out = T / stride;
        pl = 0;
    } else {
        src = x.contiguous();
        t_in = T;
        t_out = (T + pad_left + pad_right - K) / stride + 1;
        pl = pad_left;
    }
    TORCH_CHECK_VALUE(t_out > 0, "input too short");
    auto y = at::empty({B, P * t_out}, x.options());
    rave_fir_args a{};
    a.batch = (int)B; a.t_in = (int)t_in; a.t_out = (int)t_out; a.phases = (int)P; a.taps = (int)K;
    a.stride = (int)stride; a.pad_left = (int)pl;
    a.x = src.data_ptr<float>(); a.x_sb = src.stride(0);
    a.y = y.data_ptr<float>(); a.y_sb = y.stride(0);
    a.h = hd.data_ptr<float>();
    check(rave_fir(&a, c10::hip::getCurrentHIPStream(x.get_device()).stream()), "fir");
    if (hist.has_value()) {
        at::Tensor hs = *hist;
        hs.copy_(src.narrow(1, T, hs.size(1)));      // newest H samples become the cache
    }
    return y;
}

// ============================================================== operator seam
// The cc.* operators the reference's blocks construct (rave/blocks.py:65,97,
// 182,566; rave/__init__.py:14-27) and CachedPQMF's two convolutions
// (rave/pqmf.py:234-284), as torch.ops.rave_amd.* -- the kernels behind the
// rave_amd.cc nn.Modules.  Tensors on the GPU, time contiguous; launches on
// torch's current HIP stream; every op goes through the C-ABI.
void seam_tensor(const at::Tensor& t, const char* what) {
    TORCH_CHECK_VALUE(t.is_cuda() && t.scalar_type() == at::kFloat, what, " must be a float32 GPU tensor");
    TORCH_CHECK_VALUE(t.dim() == 3 && t.stride(2) == 1, what, " must be (B, C, T) with T contiguous");
}
void* cur_stream(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.get_device()).stream(); }

// rave_amd::pack_conv1d -- rave_conv1d_pack_weight / rave_conv1d_split_pack_weight
// on the host (torch layout in: Conv1d (c_out, c_in, k), ConvTranspose1d
// (c_in, c_out, k)); a CPU float tensor out
at::Tensor pack_conv1d_op(at::Tensor w, int64_t c_in, int64_t c_out, int64_t kernel, int64_t stride, int64_t dilation,
                          bool transposed, int64_t out_shift, int64_t precision) {
    TORCH_CHECK_VALUE(precision == RAVE_PREC_F32 || precision == RAVE_PREC_SPLIT16, "precision: 0 (f32) or 1 (split16)");
    at::Tensor wc = w.detach().to(at::kCPU, at::kFloat).contiguous();
    TORCH_CHECK_VALUE(wc.numel() == c_in * c_out * kernel, "weight has ", wc.numel(), " values, expected ",
                      c_in * c_out * kernel);
    const bool sp = precision == RAVE_PREC_SPLIT16;
    const int64_t n = sp ? rave_conv1d_split_packed_size((int)c_in, (int)c_out, (int)kernel, (int)stride, (int)dilation,
                                                         transposed)
                         : rave_conv1d_packed_size((int)c_in, (int)c_out, (int)kernel, (int)stride, (int)dilation,
                                                   transposed);
    TORCH_CHECK_NOT_IMPLEMENTED(n > 0, "conv1d: unsupported layer shape (c_in ", c_in, ", kernel ", kernel, ", stride ",
                                stride, ", dilation ", dilation, ")");
    at::Tensor out = at::zeros({n}, at::kFloat);
    check(sp ? rave_conv1d_split_pack_weight(wc.data_ptr<float>(), (int)c_in, (int)c_out, (int)kernel, (int)stride,
                                             (int)dilation, transposed, (int)out_shift, out.data_ptr<float>())
             : rave_conv1d_pack_weight(wc.data_ptr<float>(), (int)c_in, (int)c_out, (int)kernel, (int)stride,
                                       (int)dilation, transposed, (int)out_shift, out.data_ptr<float>()),
          "pack_conv1d");
    return out;
}

// rave_amd::conv1d_packed_size -- rave_conv1d_packed_size: floats of the exact-fp32
// image of a layer (-1: a shape the kernels do not implement)
int64_t conv1d_packed_size_op(int64_t c_in, int64_t c_out, int64_t kernel, int64_t stride, int64_t dilation,
                              bool transposed) {
    return rave_conv1d_packed_size((int)c_in, (int)c_out, (int)kernel, (int)stride, (int)dilation, transposed);
}

// rave_amd::pack_conv1d_device_ -- rave_conv1d_pack_weight_device: the exact-fp32
// image of a GPU weight into an existing GPU buffer of rave_conv1d_packed_size
// floats (every float written), one launch on torch's current stream; no host
// copy, no allocation, no synchronisation.  The weight is read detached: the
// autograd edge to it is conv1d_w's / conv_transpose1d_w's.
at::Tensor& pack_conv1d_device_op(const at::Tensor& w, at::Tensor& packed, int64_t c_in, int64_t c_out, int64_t kernel,
                                  int64_t stride, int64_t dilation, bool transposed, int64_t out_shift) {
    TORCH_CHECK_VALUE(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_contiguous(),
                      "w must be a contiguous float32 GPU tensor");
    TORCH_CHECK_VALUE(packed.is_cuda() && packed.scalar_type() == at::kFloat && packed.is_contiguous(),
                      "packed must be a contiguous float32 GPU tensor");
    TORCH_CHECK_VALUE(packed.device() == w.device(), "packed must be on w's device");
    TORCH_CHECK_VALUE(w.numel() == c_in * c_out * kernel, "weight has ", w.numel(), " values, expected ",
                      c_in * c_out * kernel);
    const int64_t n = rave_conv1d_packed_size((int)c_in, (int)c_out, (int)kernel, (int)stride, (int)dilation, transposed);
    TORCH_CHECK_NOT_IMPLEMENTED(n > 0, "conv1d: unsupported layer shape (c_in ", c_in, ", kernel ", kernel, ", stride ",
                                stride, ", dilation ", dilation, ")");
    TORCH_CHECK_VALUE(packed.numel() == n, "packed has ", packed.numel(), " values, expected ", n);
    c10::hip::HIPGuard g((c10::DeviceIndex)w.get_device());
    check(rave_conv1d_pack_weight_device(w.data_ptr<float>(), (int)c_in, (int)c_out, (int)kernel, (int)stride,
                                         (int)dilation, transposed, (int)out_shift, packed.data_ptr<float>(),
                                         cur_stream(w)),
          "pack_conv1d_device_");
    return packed;
}

// rave_amd::conv1d -- rave_conv1d: act(x) conv W (+ bias) (+ residual).
// transposed: the polyphase ConvTranspose1d (offline: pad_left 0, out_shift
// stride/2; cached: x starts with one history column, pad_left 1, out_shift 0).
at::Tensor conv1d_op(at::Tensor x, at::Tensor packed, c10::optional<at::Tensor> bias, c10::optional<at::Tensor> alpha,
                     c10::optional<at::Tensor> residual, int64_t c_out, int64_t kernel, int64_t stride, int64_t dilation,
                     int64_t pad_left, int64_t pad_right, bool transposed, int64_t out_shift, int64_t act, double slope,
                     int64_t precision) {
    seam_tensor(x, "x");
    c10::hip::HIPGuard g((c10::DeviceIndex)x.get_device());
    TORCH_CHECK_VALUE(packed.device() == x.device(), "packed weight must be on x's device");
    const int64_t B = x.size(0), c_in = x.size(1), T = x.size(2);
    int64_t t_out;
    if (transposed) {
        t_out = (T - pad_left) * stride;
    } else {
        const int64_t span = (kernel - 1) * dilation + 1;
        t_out = (T + pad_left + pad_right - span) / stride + 1;
    }
    TORCH_CHECK_VALUE(t_out > 0, "conv1d: input too short");
    at::Tensor y = at::empty({B, c_out, t_out}, x.options());
    rave_conv1d_args a{};
    a.c_in = (int)c_in; a.c_out = (int)c_out; a.kernel = (int)kernel; a.stride = (int)stride; a.dilation = (int)dilation;
    a.pad_left = (int)pad_left; a.pad_right = transposed ? 0 : (int)pad_right; a.transposed = transposed;
    a.out_shift = (int)out_shift; a.act = (int)act; a.leaky_slope = (float)slope; a.batch = (int)B;
    a.t_in = (int)T; a.t_out = (int)t_out; a.precision = (int)precision;
    a.x = x.data_ptr<float>(); a.x_sb = x.stride(0); a.x_sc = x.stride(1);
    a.y = y.data_ptr<float>(); a.y_sb = y.stride(0); a.y_sc = y.stride(1);
    at::Tensor res;
    if (residual.has_value()) {
        res = *residual;
        seam_tensor(res, "residual");
        TORCH_CHECK_VALUE(res.size(0) == B && res.size(1) == c_out && res.size(2) == t_out, "residual shape");
        a.residual = res.data_ptr<float>(); a.r_sb = res.stride(0); a.r_sc = res.stride(1);
    }
    a.weight = packed.data_ptr<float>();
    at::Tensor bd, ad;
    if (bias.has_value()) {
        bd = bias->to(x.device(), at::kFloat).contiguous();
        TORCH_CHECK_VALUE(bd.numel() == c_out, "bias must have c_out values");
        a.bias = bd.data_ptr<float>();
    }
    if (act == RAVE_ACT_SNAKE) {
        TORCH_CHECK_VALUE(alpha.has_value(), "Snake needs alpha");
        ad = alpha->to(x.device(), at::kFloat).contiguous();
        TORCH_CHECK_VALUE(ad.numel() == c_in, "alpha must have c_in values");
        a.alpha = ad.data_ptr<float>();
    }
    const int64_t nws = rave_conv1d_workspace(&a);
    if (nws < 0) check((int)nws, "conv1d workspace");
    at::Tensor ws;
    if (nws > 0) {
        ws = at::zeros({nws}, x.options());      // split-K arrival counters start (and end) zero
        a.partial = ws.data_ptr<float>();
    }
    check(rave_conv1d(&a, cur_stream(x)), "conv1d");
    return y;
}

// rave_amd::conv1d_backward -- the gradients of a non-transposed conv1d call on
// rave_conv1d_backward_data / _weight (exact fp32): gy (B, c_out, t_out), the
// forward's x (B, c_in, t_in; None where neither an activation's derivative nor
// gweight reads it), the torch-layout weight (None where neither gx nor galpha
// is asked for) and alpha -> (gx, gweight, gbias,
// galpha), each None where its bit of `need` (1 x, 2 weight, 4 bias, 8 alpha) is clear.
//
// transposed (rave_amd::conv_transpose1d_backward): the offline ConvTranspose1d(c_in, c_out,
// 2 r, stride r, padding r/2) on rave_conv_transpose1d_backward_data / _weight; the weight
// and gweight are then torch's (c_in, c_out, kernel).
using ConvGrads =
    std::tuple<c10::optional<at::Tensor>, c10::optional<at::Tensor>, c10::optional<at::Tensor>, c10::optional<at::Tensor>>;
ConvGrads conv_backward_impl(at::Tensor gy, c10::optional<at::Tensor> x_, c10::optional<at::Tensor> weight,
                             c10::optional<at::Tensor> alpha, int64_t c_in, int64_t t_in, int64_t kernel, int64_t stride,
                             int64_t dilation, int64_t pad_left, int64_t pad_right, int64_t act, double slope,
                             int64_t need, bool transposed) {
    seam_tensor(gy, "gy");
    c10::hip::HIPGuard g((c10::DeviceIndex)gy.get_device());
    const int64_t B = gy.size(0), c_out = gy.size(1), T = t_in;
    // x: needed by an activation's derivative and by gweight; weight: by gx and galpha
    const bool want_data = (need & 1) || ((need & 8) && act == RAVE_ACT_SNAKE);
    TORCH_CHECK_VALUE(x_.has_value() || !(act != RAVE_ACT_NONE && want_data) && !(need & 2),
                      "conv1d_backward: these gradients need the forward's input x");
    TORCH_CHECK_VALUE(weight.has_value() || !want_data, "conv1d_backward: gx and galpha need the weight");
    at::Tensor x, w;
    if (x_.has_value()) {
        x = *x_;
        seam_tensor(x, "x");
        TORCH_CHECK_VALUE(x.device() == gy.device() && x.size(0) == B && x.size(1) == c_in && x.size(2) == T,
                          "x must be (B, c_in, t_in) on gy's device");
    }
    if (weight.has_value()) {
        TORCH_CHECK_VALUE(weight->is_cuda() && weight->device() == gy.device() && weight->scalar_type() == at::kFloat &&
                              weight->dim() == 3 && weight->size(0) == (transposed ? c_in : c_out) &&
                              weight->size(1) == (transposed ? c_out : c_in) && weight->size(2) == kernel,
                          "weight must be a float32 ", transposed ? "(c_in, c_out, kernel)" : "(c_out, c_in, kernel)",
                          " tensor on gy's device");
        w = weight->contiguous();
    }
    rave_conv1d_backward_args a{};
    a.transposed = transposed ? 1 : 0; a.out_shift = transposed ? (int)(stride / 2) : 0;
    a.c_in = (int)c_in; a.c_out = (int)c_out; a.kernel = (int)kernel; a.stride = (int)stride; a.dilation = (int)dilation;
    a.pad_left = (int)pad_left; a.pad_right = (int)pad_right; a.act = (int)act; a.leaky_slope = (float)slope;
    a.batch = (int)B; a.t_in = (int)T; a.t_out = (int)gy.size(2); a.precision = RAVE_PREC_F32;
    if (x.defined()) {
        a.x = x.data_ptr<float>(); a.x_sb = x.stride(0); a.x_sc = x.stride(1);
    }
    a.gy = gy.data_ptr<float>(); a.gy_sb = gy.stride(0); a.gy_sc = gy.stride(1);
    if (w.defined()) a.weight = w.data_ptr<float>();
    at::Tensor ad;
    const bool snake = act == RAVE_ACT_SNAKE;
    if (snake) {
        TORCH_CHECK_VALUE(alpha.has_value(), "Snake needs alpha");
        ad = alpha->to(gy.device(), at::kFloat).contiguous();
        TORCH_CHECK_VALUE(ad.numel() == c_in, "alpha must have c_in values");
        a.alpha = ad.data_ptr<float>();
    }
    c10::optional<at::Tensor> gx, gw, gb, ga;
    if ((need & 1)) {
        gx = at::empty({B, c_in, T}, gy.options());
        a.gx = gx->data_ptr<float>(); a.gx_sb = gx->stride(0); a.gx_sc = gx->stride(1);
    }
    if ((need & 2)) {
        gw = transposed ? at::empty({c_in, c_out, kernel}, gy.options()) : at::empty({c_out, c_in, kernel}, gy.options());
        a.gweight = gw->data_ptr<float>();
    }
    if ((need & 4)) {
        gb = at::empty({c_out}, gy.options());
        a.gbias = gb->data_ptr<float>();
    }
    if ((need & 8) && snake) {
        ga = at::empty({c_in}, gy.options());
        a.galpha = ga->data_ptr<float>();
    }
    const int64_t nws = transposed ? rave_conv_transpose1d_backward_workspace(&a) : rave_conv1d_backward_workspace(&a);
    if (nws < 0) check((int)nws, transposed ? "conv_transpose1d_backward" : "conv1d_backward");
    at::Tensor ws;
    if (nws > 0) {
        ws = at::empty({nws}, gy.options());                 // slabs and partials: nothing to zero
        a.workspace = ws.data_ptr<float>();
    }
    if (transposed) {
        check(rave_conv_transpose1d_backward_data(&a, cur_stream(gy)), "conv_transpose1d_backward_data");
        check(rave_conv_transpose1d_backward_weight(&a, cur_stream(gy)), "conv_transpose1d_backward_weight");
    } else {
        check(rave_conv1d_backward_data(&a, cur_stream(gy)), "conv1d_backward_data");
        check(rave_conv1d_backward_weight(&a, cur_stream(gy)), "conv1d_backward_weight");
    }
    return std::make_tuple(gx, gw, gb, ga);
}

ConvGrads conv1d_backward_op(at::Tensor gy, c10::optional<at::Tensor> x, c10::optional<at::Tensor> weight,
                             c10::optional<at::Tensor> alpha, int64_t c_in, int64_t t_in, int64_t kernel, int64_t stride,
                             int64_t dilation, int64_t pad_left, int64_t pad_right, int64_t act, double slope,
                             int64_t need) {
    return conv_backward_impl(gy, x, weight, alpha, c_in, t_in, kernel, stride, dilation, pad_left, pad_right, act, slope,
                              need, false);
}

ConvGrads conv_transpose1d_backward_op(at::Tensor gy, c10::optional<at::Tensor> x, c10::optional<at::Tensor> weight,
                                       c10::optional<at::Tensor> alpha, int64_t c_in, int64_t t_in, int64_t kernel,
                                       int64_t stride, int64_t act, double slope, int64_t need) {
    return conv_backward_impl(gy, x, weight, alpha, c_in, t_in, kernel, stride, 1, 0, 0, act, slope, need, true);
}

// rave_amd::conv1d_w -- conv1d with the torch-layout weight beside its packed
// image, so autograd has an edge to the parameter: the plain kernel is conv1d_op
// itself (same launch, same bits; `weight` is not read), the autograd
// implementation below sends the cotangent through conv1d_backward.
// Non-transposed convs only.
at::Tensor conv1d_w_op(at::Tensor x, at::Tensor weight, at::Tensor packed, c10::optional<at::Tensor> bias,
                       c10::optional<at::Tensor> alpha, c10::optional<at::Tensor> residual, int64_t c_out,
                       int64_t kernel, int64_t stride, int64_t dilation, int64_t pad_left, int64_t pad_right,
                       int64_t act, double slope, int64_t precision) {
    (void)weight;
    return conv1d_op(x, packed, bias, alpha, residual, c_out, kernel, stride, dilation, pad_left, pad_right, false, 0,
                     act, slope, precision);
}

// rave_amd::conv_transpose1d_w -- the same for the offline ConvTranspose1d(c_in, c_out, 2 r,
// stride r, padding r/2): conv1d_op's transposed launch on the packed image (out_shift
// stride/2), with the torch-layout (c_in, c_out, kernel) weight beside it for autograd.
at::Tensor conv_transpose1d_w_op(at::Tensor x, at::Tensor weight, at::Tensor packed, c10::optional<at::Tensor> bias,
                                 c10::optional<at::Tensor> alpha, c10::optional<at::Tensor> residual, int64_t c_out,
                                 int64_t kernel, int64_t stride, int64_t act, double slope, int64_t precision) {
    (void)weight;
    return conv1d_op(x, packed, bias, alpha, residual, c_out, kernel, stride, 1, 0, 0, true, stride / 2, act, slope,
                     precision);
}

// rave_amd::pqmf_analysis -- CachedPQMF.forward (rave/pqmf.py:269-273): x (B, 1, T)
// -> (B, n_out_bands, T / n_band); hkf (n_band, taps) on x's device
at::Tensor pqmf_analysis_op(at::Tensor x, at::Tensor hkf, int64_t n_out_bands, int64_t pad_left, int64_t precision) {
    seam_tensor(x, "x");
    c10::hip::HIPGuard g((c10::DeviceIndex)x.get_device());
    TORCH_CHECK_VALUE(x.size(1) == 1, "x must be (B, 1, T)");
    at::Tensor h = hkf.to(x.device(), at::kFloat).contiguous();
    const int64_t nb = h.size(0), B = x.size(0), T = x.size(2);
    TORCH_CHECK_VALUE(T % nb == 0, "T must be a multiple of n_band");
    at::Tensor y = at::empty({B, n_out_bands, T / nb}, x.options());
    rave_pqmf_analysis_args a{};
    a.n_band = (int)nb; a.taps = (int)h.size(1); a.n_out_bands = (int)n_out_bands; a.batch = (int)B;
    a.t_in = (int)T; a.pad_left = (int)pad_left; a.t_out = (int)(T / nb); a.precision = (int)precision;
    a.x = x.data_ptr<float>(); a.x_sb = x.stride(0);
    a.y = y.data_ptr<float>(); a.y_sb = y.stride(0); a.y_sc = y.stride(1);
    a.hkf = h.data_ptr<float>();
    check(rave_pqmf_analysis(&a, cur_stream(x)), "pqmf_analysis");
    return y;
}

// rave_amd::pqmf_synthesis -- CachedPQMF.inverse (rave/pqmf.py:275-284): x (B, n_band, F)
// -> (B, 1, F * n_band); hki (n_band, n_band, taps).  x_len > F: x carries
// cached history columns before the F frames (streaming, pad_left 0).
// mode 1 / 2: GeneratorV2's epilogue fused in front (rave/blocks.py:699-707):
// x holds 2 n_band channels (waveform, amplitude) and the input is
// tanh(x[:n] * sigmoid(x[n:]) + noise) (mode 1) or tanh(x + noise) (mode 2);
// noise (B, n_band, x_len) or None.
at::Tensor pqmf_synthesis_op(at::Tensor x, at::Tensor hki, int64_t pad_left, int64_t frames, int64_t frame0,
                             int64_t precision, int64_t mode, c10::optional<at::Tensor> noise) {
    seam_tensor(x, "x");
    c10::hip::HIPGuard g((c10::DeviceIndex)x.get_device());
    at::Tensor h = hki.to(x.device(), at::kFloat).contiguous();
    const int64_t nb = h.size(0), B = x.size(0), XL = x.size(2);
    TORCH_CHECK_VALUE(mode >= 0 && mode <= 2, "mode must be 0 (plain), 1 (amplitude modulation) or 2 (tanh)");
    TORCH_CHECK_VALUE(x.size(1) == (mode == 1 ? 2 * nb : nb), "x must have ", mode == 1 ? 2 * nb : nb, " channels");
    TORCH_CHECK_VALUE(mode != 0 || !noise.has_value(), "noise needs an epilogue mode");
    const int64_t F = frames > 0 ? frames : XL;
    at::Tensor y = at::empty({B, 1, F * nb}, x.options());
    rave_pqmf_synthesis_args a{};
    a.n_band = (int)nb; a.taps = (int)h.size(2); a.batch = (int)B; a.t_in = (int)F; a.pad_left = (int)pad_left;
    a.mode = (int)mode; a.frame0 = (int)frame0; a.x_len = (int)XL;
    a.x = x.data_ptr<float>(); a.x_sb = x.stride(0); a.x_sc = x.stride(1);
    at::Tensor nz;
    if (noise.has_value()) {
        nz = *noise;
        seam_tensor(nz, "noise");
        TORCH_CHECK_VALUE(nz.dim() == 3 && nz.size(0) == B && nz.size(1) == nb && nz.size(2) == XL && nz.stride(2) == 1,
                          "noise must be (B, n_band, x_len), time contiguous");
        a.noise = nz.data_ptr<float>(); a.n_sb = nz.stride(0); a.n_sc = nz.stride(1);
    }
    a.y = y.data_ptr<float>(); a.y_sb = y.stride(0);
    a.hki = h.data_ptr<float>(); a.precision = (int)precision;
    check(rave_pqmf_synthesis(&a, cur_stream(x)), "pqmf_synthesis");
    return y;
}

// rave_amd::pqmf_analysis_backward -- the adjoint of pqmf_analysis on
// rave_pqmf_analysis_backward: gy (B, n_out_bands, t_out) -> gx (B, 1, t_in)
at::Tensor pqmf_analysis_backward_op(at::Tensor gy, at::Tensor hkf, int64_t n_out_bands, int64_t pad_left,
                                     int64_t t_in) {
    seam_tensor(gy, "gy");
    c10::hip::HIPGuard g((c10::DeviceIndex)gy.get_device());
    TORCH_CHECK_VALUE(gy.size(1) == n_out_bands, "gy must be (B, n_out_bands, t_out)");
    at::Tensor h = hkf.to(gy.device(), at::kFloat).contiguous();
    const int64_t B = gy.size(0);
    at::Tensor gx = at::empty({B, 1, t_in}, gy.options());
    rave_pqmf_analysis_backward_args a{};
    a.n_band = (int)h.size(0); a.taps = (int)h.size(1); a.n_out_bands = (int)n_out_bands; a.batch = (int)B;
    a.t_in = (int)t_in; a.pad_left = (int)pad_left; a.t_out = (int)gy.size(2); a.precision = RAVE_PREC_F32;
    a.gy = gy.data_ptr<float>(); a.gy_sb = gy.stride(0); a.gy_sc = gy.stride(1);
    a.gx = gx.data_ptr<float>(); a.gx_sb = gx.stride(0);
    a.hkf = h.data_ptr<float>();
    check(rave_pqmf_analysis_backward(&a, cur_stream(gy)), "pqmf_analysis_backward");
    return gx;
}

// rave_amd::pqmf_synthesis_backward -- the adjoint of pqmf_synthesis with the
// epilogue's derivative (rave_pqmf_synthesis_backward): gy (B, 1, F n_band) and
// the forward call's x / noise -> gx like x, gnoise like noise (None without)
std::tuple<at::Tensor, c10::optional<at::Tensor>> pqmf_synthesis_backward_op(
    at::Tensor gy, at::Tensor x, at::Tensor hki, int64_t pad_left, int64_t frames, int64_t frame0, int64_t x_len,
    int64_t mode, c10::optional<at::Tensor> noise) {
    seam_tensor(gy, "gy");
    seam_tensor(x, "x");
    c10::hip::HIPGuard g((c10::DeviceIndex)x.get_device());
    at::Tensor h = hki.to(x.device(), at::kFloat).contiguous();
    const int64_t nb = h.size(0), B = x.size(0), XL = x.size(2);
    TORCH_CHECK_VALUE(mode >= 0 && mode <= 2, "mode must be 0 (plain), 1 (amplitude modulation) or 2 (tanh)");
    TORCH_CHECK_VALUE(x.size(1) == (mode == 1 ? 2 * nb : nb), "x must have ", mode == 1 ? 2 * nb : nb, " channels");
    TORCH_CHECK_VALUE(mode != 0 || !noise.has_value(), "noise needs an epilogue mode");
    TORCH_CHECK_VALUE(x_len == XL, "x_len must be x's length");
    const int64_t F = frames > 0 ? frames : XL;
    TORCH_CHECK_VALUE(gy.size(0) == B && gy.size(1) == 1 && gy.size(2) == F * nb, "gy must be (B, 1, frames n_band)");
    at::Tensor gx = at::empty({B, x.size(1), XL}, x.options());
    rave_pqmf_synthesis_backward_args a{};
    a.n_band = (int)nb; a.taps = (int)h.size(2); a.batch = (int)B; a.t_in = (int)F; a.pad_left = (int)pad_left;
    a.mode = (int)mode; a.frame0 = (int)frame0; a.x_len = (int)XL;
    a.gy = gy.data_ptr<float>(); a.gy_sb = gy.stride(0);
    a.x = x.data_ptr<float>(); a.x_sb = x.stride(0); a.x_sc = x.stride(1);
    a.gx = gx.data_ptr<float>(); a.gx_sb = gx.stride(0); a.gx_sc = gx.stride(1);
    c10::optional<at::Tensor> gnoise;
    at::Tensor nz, gn;
    if (noise.has_value()) {
        nz = *noise;
        seam_tensor(nz, "noise");
        TORCH_CHECK_VALUE(nz.size(0) == B && nz.size(1) == nb && nz.size(2) == XL,
                          "noise must be (B, n_band, x_len), time contiguous");
        gn = at::empty({B, nb, XL}, x.options());
        a.noise = nz.data_ptr<float>(); a.n_sb = nz.stride(0); a.n_sc = nz.stride(1);
        a.gnoise = gn.data_ptr<float>(); a.gn_sb = gn.stride(0); a.gn_sc = gn.stride(1);
        gnoise = gn;
    }
    a.hki = h.data_ptr<float>(); a.precision = RAVE_PREC_F32;
    check(rave_pqmf_synthesis_backward(&a, cur_stream(x)), "pqmf_synthesis_backward");
    return std::make_tuple(gx, gnoise);
}

// Autograd for the two PQMF ops (registered on the autograd key below, so
// scripted modules and TorchScript hosts get it too): the forward is the op
// itself; the backward is one adjoint call.  The filters are constants (no
// gradient); exact fp32 only; no double backward.
void no_double_backward(const char* op) {
    TORCH_CHECK_NOT_IMPLEMENTED(!at::GradMode::is_enabled(), op, ": double backward is not implemented");
}

struct PqmfAnalysisFn : torch::autograd::Function<PqmfAnalysisFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, at::Tensor x, at::Tensor hkf, int64_t n_out_bands,
                              int64_t pad_left, int64_t precision) {
        at::AutoDispatchBelowADInplaceOrView below;
        ctx->save_for_backward({hkf});
        ctx->saved_data["n_out_bands"] = n_out_bands;
        ctx->saved_data["pad_left"] = pad_left;
        ctx->saved_data["t_in"] = x.size(2);
        return pqmf_analysis_op(x, hkf, n_out_bands, pad_left, precision);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                   torch::autograd::variable_list grads) {
        no_double_backward("pqmf_analysis");
        at::AutoDispatchBelowADInplaceOrView below;
        const auto saved = ctx->get_saved_variables();
        at::Tensor gx = pqmf_analysis_backward_op(grads[0].contiguous(), saved[0], ctx->saved_data["n_out_bands"].toInt(),
                                                  ctx->saved_data["pad_left"].toInt(), ctx->saved_data["t_in"].toInt());
        return {gx, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

struct PqmfSynthesisFn : torch::autograd::Function<PqmfSynthesisFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, at::Tensor x, at::Tensor hki, int64_t pad_left,
                              int64_t frames, int64_t frame0, int64_t precision, int64_t mode,
                              c10::optional<at::Tensor> noise) {
        at::AutoDispatchBelowADInplaceOrView below;
        ctx->save_for_backward({x, hki, noise.has_value() ? *noise : at::Tensor()});
        ctx->saved_data["pad_left"] = pad_left;
        ctx->saved_data["frames"] = frames;
        ctx->saved_data["frame0"] = frame0;
        ctx->saved_data["mode"] = mode;
        return pqmf_synthesis_op(x, hki, pad_left, frames, frame0, precision, mode, noise);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                   torch::autograd::variable_list grads) {
        no_double_backward("pqmf_synthesis");
        at::AutoDispatchBelowADInplaceOrView below;
        const auto saved = ctx->get_saved_variables();
        c10::optional<at::Tensor> noise;
        if (saved[2].defined()) noise = saved[2];
        auto g = pqmf_synthesis_backward_op(grads[0].contiguous(), saved[0], saved[1],
                                            ctx->saved_data["pad_left"].toInt(), ctx->saved_data["frames"].toInt(),
                                            ctx->saved_data["frame0"].toInt(), saved[0].size(2),
                                            ctx->saved_data["mode"].toInt(), noise);
        at::Tensor gn = std::get<1>(g).has_value() ? *std::get<1>(g) : at::Tensor();
        return {std::get<0>(g), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), gn};
    }
};

bool wants_grad(const at::Tensor& x, const c10::optional<at::Tensor>& other, int64_t precision, const char* op) {
    if (!at::GradMode::is_enabled() || !(x.requires_grad() || (other.has_value() && other->requires_grad())))
        return false;
    TORCH_CHECK_NOT_IMPLEMENTED(precision == RAVE_PREC_F32, op,
                                ": only the exact fp32 precision (0) is differentiable; got precision ", precision,
                                " with an input that requires grad");
    return true;
}

at::Tensor pqmf_analysis_autograd(at::Tensor x, at::Tensor hkf, int64_t n_out_bands, int64_t pad_left,
                                  int64_t precision) {
    if (wants_grad(x, c10::nullopt, precision, "pqmf_analysis")) {
        seam_tensor(x, "x");
        return PqmfAnalysisFn::apply(x, hkf, n_out_bands, pad_left, precision);
    }
    at::AutoDispatchBelowADInplaceOrView below;
    return pqmf_analysis_op(x, hkf, n_out_bands, pad_left, precision);
}

at::Tensor pqmf_synthesis_autograd(at::Tensor x, at::Tensor hki, int64_t pad_left, int64_t frames, int64_t frame0,
                                   int64_t precision, int64_t mode, c10::optional<at::Tensor> noise) {
    if (wants_grad(x, noise, precision, "pqmf_synthesis")) {
        seam_tensor(x, "x");
        return PqmfSynthesisFn::apply(x, hki, pad_left, frames, frame0, precision, mode, noise);
    }
    at::AutoDispatchBelowADInplaceOrView below;
    return pqmf_synthesis_op(x, hki, pad_left, frames, frame0, precision, mode, noise);
}

// Autograd for conv1d_w and conv_transpose1d_w (`transposed`; dilation 1 and no padding
// arguments there): saves x, the weight and alpha; one backward op call
// returns the gradients of x, weight, bias and alpha, and the residual gets the
// cotangent itself.  Exact fp32 only; no double backward.
struct Conv1dWFn : torch::autograd::Function<Conv1dWFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, at::Tensor x, at::Tensor weight, at::Tensor packed,
                              c10::optional<at::Tensor> bias, c10::optional<at::Tensor> alpha,
                              c10::optional<at::Tensor> residual, int64_t c_out, int64_t kernel, int64_t stride,
                              int64_t dilation, int64_t pad_left, int64_t pad_right, int64_t act, double slope,
                              int64_t precision, bool transposed) {
        at::AutoDispatchBelowADInplaceOrView below;
        // only what the backward can read: x for an activation's derivative (when x or alpha
        // takes a gradient) and for gweight; the weight for gx and galpha
        const bool snake = act == RAVE_ACT_SNAKE && alpha.has_value();
        const bool data = x.requires_grad() || (snake && alpha->requires_grad());
        const bool keep_x = weight.requires_grad() || (act != RAVE_ACT_NONE && data);
        ctx->save_for_backward({keep_x ? x : at::Tensor(), data ? weight : at::Tensor(), snake ? *alpha : at::Tensor()});
        ctx->saved_data["c_in"] = x.size(1);
        ctx->saved_data["t_in"] = x.size(2);
        ctx->saved_data["kernel"] = kernel;
        ctx->saved_data["stride"] = stride;
        ctx->saved_data["dilation"] = dilation;
        ctx->saved_data["pad_left"] = pad_left;
        ctx->saved_data["pad_right"] = pad_right;
        ctx->saved_data["act"] = act;
        ctx->saved_data["slope"] = slope;
        ctx->saved_data["has_bias"] = bias.has_value();
        ctx->saved_data["has_res"] = residual.has_value();
        ctx->saved_data["has_alpha"] = alpha.has_value();
        ctx->saved_data["transposed"] = transposed;
        if (transposed)
            return conv_transpose1d_w_op(x, weight, packed, bias, alpha, residual, c_out, kernel, stride, act, slope,
                                         precision);
        return conv1d_w_op(x, weight, packed, bias, alpha, residual, c_out, kernel, stride, dilation, pad_left, pad_right,
                           act, slope, precision);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                   torch::autograd::variable_list grads) {
        const bool transposed = ctx->saved_data["transposed"].toBool();
        no_double_backward(transposed ? "conv_transpose1d_w" : "conv1d_w");
        at::AutoDispatchBelowADInplaceOrView below;
        const auto saved = ctx->get_saved_variables();
        c10::optional<at::Tensor> alpha;
        if (saved[2].defined()) alpha = saved[2];
        const bool has_bias = ctx->saved_data["has_bias"].toBool(), has_res = ctx->saved_data["has_res"].toBool();
        // needs_input_grad counts the tensors that were passed (an absent optional has no edge):
        // x, weight, packed, then bias, alpha and residual where given
        const bool has_alpha = ctx->saved_data["has_alpha"].toBool();
        const int e_bias = 3, e_alpha = e_bias + (has_bias ? 1 : 0), e_res = e_alpha + (has_alpha ? 1 : 0);
        const int64_t need = (ctx->needs_input_grad(0) ? 1 : 0) | (ctx->needs_input_grad(1) ? 2 : 0) |
                             (has_bias && ctx->needs_input_grad(e_bias) ? 4 : 0) |
                             (alpha.has_value() && ctx->needs_input_grad(e_alpha) ? 8 : 0);
        at::Tensor gy = grads[0].contiguous();
        auto opt = [](const at::Tensor& t) { return t.defined() ? c10::optional<at::Tensor>(t) : c10::nullopt; };
        auto g = conv_backward_impl(gy, opt(saved[0]), opt(saved[1]), alpha, ctx->saved_data["c_in"].toInt(),
                                    ctx->saved_data["t_in"].toInt(), ctx->saved_data["kernel"].toInt(),
                                    ctx->saved_data["stride"].toInt(), ctx->saved_data["dilation"].toInt(),
                                    ctx->saved_data["pad_left"].toInt(), ctx->saved_data["pad_right"].toInt(),
                                    ctx->saved_data["act"].toInt(), ctx->saved_data["slope"].toDouble(), need,
                                    transposed);
        auto get = [](const c10::optional<at::Tensor>& t) { return t.has_value() ? *t : at::Tensor(); };
        torch::autograd::variable_list out(16);
        out[0] = get(std::get<0>(g));
        out[1] = get(std::get<1>(g));
        out[3] = get(std::get<2>(g));
        out[4] = get(std::get<3>(g));
        if (has_res && ctx->needs_input_grad(e_res)) out[5] = gy;
        return out;
    }
};

at::Tensor conv1d_w_autograd(at::Tensor x, at::Tensor weight, at::Tensor packed, c10::optional<at::Tensor> bias,
                             c10::optional<at::Tensor> alpha, c10::optional<at::Tensor> residual, int64_t c_out,
                             int64_t kernel, int64_t stride, int64_t dilation, int64_t pad_left, int64_t pad_right,
                             int64_t act, double slope, int64_t precision) {
    auto rg = [](const c10::optional<at::Tensor>& t) { return t.has_value() && t->requires_grad(); };
    const bool any = x.requires_grad() || weight.requires_grad() || rg(bias) || rg(alpha) || rg(residual);
    if (at::GradMode::is_enabled() && any) {
        TORCH_CHECK_NOT_IMPLEMENTED(precision == RAVE_PREC_F32,
                                    "conv1d_w: only the exact fp32 precision (0) is differentiable; got precision ",
                                    precision, " with an input that requires grad");
        seam_tensor(x, "x");
        return Conv1dWFn::apply(x, weight, packed, bias, alpha, residual, c_out, kernel, stride, dilation, pad_left,
                                pad_right, act, slope, precision, false);
    }
    at::AutoDispatchBelowADInplaceOrView below;
    return conv1d_w_op(x, weight, packed, bias, alpha, residual, c_out, kernel, stride, dilation, pad_left, pad_right, act,
                       slope, precision);
}

at::Tensor conv_transpose1d_w_autograd(at::Tensor x, at::Tensor weight, at::Tensor packed, c10::optional<at::Tensor> bias,
                                       c10::optional<at::Tensor> alpha, c10::optional<at::Tensor> residual, int64_t c_out,
                                       int64_t kernel, int64_t stride, int64_t act, double slope, int64_t precision) {
    auto rg = [](const c10::optional<at::Tensor>& t) { return t.has_value() && t->requires_grad(); };
    const bool any = x.requires_grad() || weight.requires_grad() || rg(bias) || rg(alpha) || rg(residual);
    if (at::GradMode::is_enabled() && any) {
        TORCH_CHECK_NOT_IMPLEMENTED(precision == RAVE_PREC_F32,
                                    "conv_transpose1d_w: only the exact fp32 precision (0) is differentiable; got "
                                    "precision ", precision, " with an input that requires grad");
        seam_tensor(x, "x");
        return Conv1dWFn::apply(x, weight, packed, bias, alpha, residual, c_out, kernel, stride, 1, 0, 0, act, slope,
                                precision, true);
    }
    at::AutoDispatchBelowADInplaceOrView below;
    return conv_transpose1d_w_op(x, weight, packed, bias, alpha, residual, c_out, kernel, stride, act, slope, precision);
}

// rave_amd::adain -- AdaptiveInstanceNormalization.forward in eval mode
// (rave/blocks.py:856-919) on rave_adain over the module's own buffers
// (mean_x / std_x / mean_y / std_y (max_batch, C, 1), num_update_x / _y (1,)):
// mode 0 transfer (when both counters are set), 1 learn_x then transfer,
// 2 learn_y; a learning mode writes the updated statistics back.
// `kept` (autograd's forward) receives the call's own (4, max_batch, C) statistics
// and (2,) counters as the kernel left them: post-update copies nobody else holds.
at::Tensor adain_impl(at::Tensor x, at::Tensor mean_x, at::Tensor std_x, at::Tensor mean_y, at::Tensor std_y,
                      at::Tensor num_update_x, at::Tensor num_update_y, int64_t mode,
                      std::pair<at::Tensor, at::Tensor>* kept) {
    seam_tensor(x, "x");
    TORCH_CHECK_VALUE(x.dim() == 3, "x must be (B, C, T)");
    TORCH_CHECK_VALUE(mode >= 0 && mode <= 2, "mode must be 0 (transfer), 1 (learn_x) or 2 (learn_y)");
    c10::hip::HIPGuard g((c10::DeviceIndex)x.get_device());
    const int64_t B = x.size(0), C = x.size(1), T = x.size(2), mb = mean_x.size(0);
    for (const at::Tensor* t : {&mean_x, &std_x, &mean_y, &std_y})
        TORCH_CHECK_VALUE(t->dim() == 3 && t->size(0) == mb && t->size(1) == C && t->size(2) == 1,
                          "AdaIN statistics must be (max_batch, C, 1)");
    TORCH_CHECK_VALUE(B <= mb, "batch exceeds the AdaIN buffers' max_batch");
    TORCH_CHECK_VALUE(T >= 2 || mode == 0, "learning needs at least 2 samples (unbiased std)");
    at::Tensor xc = x.contiguous();
    at::Tensor stats = at::stack({mean_x, std_x, mean_y, std_y}).to(x.device(), at::kFloat).reshape({4, mb, C})
                           .contiguous();
    at::Tensor cnt = at::cat({num_update_x.reshape({1}), num_update_y.reshape({1})}).to(x.device(), at::kFloat)
                         .contiguous();
    at::Tensor ticket = at::zeros({1}, x.options().dtype(at::kInt));
    at::Tensor y = at::empty_like(xc);
    rave_adain_args a{};
    a.batch = (int)B; a.channels = (int)C; a.t_len = (int)T; a.mode = (int)mode; a.max_batch = (int)mb; a.row0 = 0;
    a.x = xc.data_ptr<float>(); a.x_sb = xc.stride(0); a.x_sc = xc.stride(1);
    a.y = y.data_ptr<float>(); a.y_sb = y.stride(0); a.y_sc = y.stride(1);
    a.stats = stats.data_ptr<float>();
    a.counters = cnt.data_ptr<float>();
    a.ticket = reinterpret_cast<uint32_t*>(ticket.data_ptr<int32_t>());
    check(rave_adain(&a, cur_stream(x)), "adain");
    if (mode == 1) {
        mean_x.copy_(stats[0].reshape(mean_x.sizes()));
        std_x.copy_(stats[1].reshape(std_x.sizes()));
        num_update_x.copy_(cnt.narrow(0, 0, 1).reshape(num_update_x.sizes()));
    } else if (mode == 2) {
        mean_y.copy_(stats[2].reshape(mean_y.sizes()));
        std_y.copy_(stats[3].reshape(std_y.sizes()));
        num_update_y.copy_(cnt.narrow(0, 1, 1).reshape(num_update_y.sizes()));
    }
    if (kept) *kept = {stats, cnt};
    return y;
}

at::Tensor adain_op(at::Tensor x, at::Tensor mean_x, at::Tensor std_x, at::Tensor mean_y, at::Tensor std_y,
                    at::Tensor num_update_x, at::Tensor num_update_y, int64_t mode) {
    return adain_impl(x, mean_x, std_x, mean_y, std_y, num_update_x, num_update_y, mode, nullptr);
}

// rave_amd::adain_backward -- the gradient of adain with respect to x on
// rave_adain_backward: gy (B, C, T), stats (4, max_batch, C) and counters (2,)
// as they stood after the forward call -> gx like gy.  The kernel reads the
// counters on the device; nothing here waits for them.
at::Tensor adain_backward_op(at::Tensor gy, at::Tensor stats, at::Tensor counters, int64_t mode) {
    seam_tensor(gy, "gy");
    TORCH_CHECK_VALUE(gy.dim() == 3, "gy must be (B, C, T)");
    TORCH_CHECK_VALUE(mode >= 0 && mode <= 2, "mode must be 0 (transfer), 1 (learn_x) or 2 (learn_y)");
    c10::hip::HIPGuard g((c10::DeviceIndex)gy.get_device());
    const int64_t B = gy.size(0), C = gy.size(1), T = gy.size(2);
    TORCH_CHECK_VALUE(stats.dim() == 3 && stats.size(0) == 4 && stats.size(2) == C,
                      "stats must be (4, max_batch, C)");
    TORCH_CHECK_VALUE(counters.numel() == 2, "counters must hold num_update_x and num_update_y");
    const int64_t mb = stats.size(1);
    TORCH_CHECK_VALUE(B <= mb, "batch exceeds the AdaIN buffers' max_batch");
    at::Tensor st = stats.to(gy.device(), at::kFloat).contiguous();
    at::Tensor cnt = counters.to(gy.device(), at::kFloat).reshape({2}).contiguous();
    at::Tensor gc = gy.contiguous();
    at::Tensor gx = at::empty_like(gc);
    rave_adain_backward_args a{};
    a.batch = (int)B; a.channels = (int)C; a.t_len = (int)T; a.mode = (int)mode; a.max_batch = (int)mb; a.row0 = 0;
    a.gy = gc.data_ptr<float>(); a.gy_sb = gc.stride(0); a.gy_sc = gc.stride(1);
    a.gx = gx.data_ptr<float>(); a.gx_sb = gx.stride(0); a.gx_sc = gx.stride(1);
    a.stats = st.data_ptr<float>();
    a.counters = cnt.data_ptr<float>();
    check(rave_adain_backward(&a, cur_stream(gy)), "adain_backward");
    return gx;
}

// rave_amd::noise_synth -- NoiseGeneratorV2's filter stage after its conv stack
// (rave/blocks.py:281-291, rave/core.py:66-129) on rave_noise_synth: amp
// (B, n_band * noise_bands, F) pre-sigmoid, u (B, F, n_band, target) U[0,1)
// (torch.rand_like(ir)) -> noise (B, n_band, F * target).
at::Tensor noise_synth_op(at::Tensor amp, at::Tensor u, int64_t n_band, int64_t noise_bands) {
    seam_tensor(amp, "amp");
    TORCH_CHECK_VALUE(u.is_cuda() && u.scalar_type() == at::kFloat, "u must be a float32 GPU tensor");
    c10::hip::HIPGuard g((c10::DeviceIndex)amp.get_device());
    TORCH_CHECK_VALUE(amp.dim() == 3 && amp.size(1) == n_band * noise_bands, "amp must be (B, n_band * noise_bands, F)");
    const int64_t B = amp.size(0), F = amp.size(2);
    TORCH_CHECK_VALUE(u.dim() == 4 && u.size(0) == B && u.size(1) == F && u.size(2) == n_band,
                      "u must be (B, F, n_band, target)");
    const int64_t target = u.size(3);
    at::Tensor ac = amp.contiguous(), uc = u.contiguous();
    at::Tensor y = at::empty({B, n_band, F * target}, amp.options());
    rave_noise_args a{};
    a.batch = (int)B; a.frames = (int)F; a.n_band = (int)n_band; a.noise_bands = (int)noise_bands;
    a.target = (int)target;
    a.amp = ac.data_ptr<float>(); a.a_sb = ac.stride(0); a.a_sc = ac.stride(1);
    a.u = uc.data_ptr<float>(); a.u_sb = uc.stride(0);
    a.y = y.data_ptr<float>(); a.y_sb = y.stride(0); a.y_sc = y.stride(1);
    check(rave_noise_synth(&a, cur_stream(amp)), "noise_synth");
    return y;
}

// rave_amd::noise_synth_backward -- the gradient of noise_synth with respect to
// amp on rave_noise_synth_backward: gy (B, n_band, F * target) and the forward
// call's amp / u -> gamp like amp.  u is a constant (the reference's rand_like).
at::Tensor noise_synth_backward_op(at::Tensor gy, at::Tensor amp, at::Tensor u, int64_t n_band, int64_t noise_bands) {
    seam_tensor(gy, "gy");
    seam_tensor(amp, "amp");
    TORCH_CHECK_VALUE(u.is_cuda() && u.scalar_type() == at::kFloat, "u must be a float32 GPU tensor");
    c10::hip::HIPGuard g((c10::DeviceIndex)amp.get_device());
    TORCH_CHECK_VALUE(amp.dim() == 3 && amp.size(1) == n_band * noise_bands, "amp must be (B, n_band * noise_bands, F)");
    const int64_t B = amp.size(0), F = amp.size(2);
    TORCH_CHECK_VALUE(u.dim() == 4 && u.size(0) == B && u.size(1) == F && u.size(2) == n_band,
                      "u must be (B, F, n_band, target)");
    const int64_t target = u.size(3);
    TORCH_CHECK_VALUE(gy.dim() == 3 && gy.size(0) == B && gy.size(1) == n_band && gy.size(2) == F * target,
                      "gy must be (B, n_band, F * target)");
    at::Tensor ac = amp.contiguous(), uc = u.contiguous(), gc = gy.contiguous();
    at::Tensor gamp = at::empty({B, n_band * noise_bands, F}, amp.options());
    rave_noise_backward_args a{};
    a.batch = (int)B; a.frames = (int)F; a.n_band = (int)n_band; a.noise_bands = (int)noise_bands;
    a.target = (int)target;
    a.amp = ac.data_ptr<float>(); a.a_sb = ac.stride(0); a.a_sc = ac.stride(1);
    a.u = uc.data_ptr<float>(); a.u_sb = uc.stride(0);
    a.gy = gc.data_ptr<float>(); a.gy_sb = gc.stride(0); a.gy_sc = gc.stride(1);
    a.gamp = gamp.data_ptr<float>(); a.ga_sb = gamp.stride(0); a.ga_sc = gamp.stride(1);
    check(rave_noise_synth_backward(&a, cur_stream(amp)), "noise_synth_backward");
    return gamp;
}

// Autograd for noise_synth and adain, in the manner of the PQMF ops: the forward is
// the op itself, the backward one kernel call; no double backward.  noise_synth
// keeps amp and u (u is a constant: asking for its gradient is refused); adain keeps
// the post-update statistics and counters its call built, never x -- the buffers and
// the statistics are constants in every mode.
struct NoiseSynthFn : torch::autograd::Function<NoiseSynthFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, at::Tensor amp, at::Tensor u, int64_t n_band,
                              int64_t noise_bands) {
        at::AutoDispatchBelowADInplaceOrView below;
        ctx->save_for_backward({amp, u});
        ctx->saved_data["n_band"] = n_band;
        ctx->saved_data["noise_bands"] = noise_bands;
        return noise_synth_op(amp, u, n_band, noise_bands);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                   torch::autograd::variable_list grads) {
        no_double_backward("noise_synth");
        at::AutoDispatchBelowADInplaceOrView below;
        const auto saved = ctx->get_saved_variables();
        at::Tensor gamp = noise_synth_backward_op(grads[0].contiguous(), saved[0], saved[1],
                                                  ctx->saved_data["n_band"].toInt(),
                                                  ctx->saved_data["noise_bands"].toInt());
        return {gamp, at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

struct AdainFn : torch::autograd::Function<AdainFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, at::Tensor x, at::Tensor mean_x, at::Tensor std_x,
                              at::Tensor mean_y, at::Tensor std_y, at::Tensor num_update_x, at::Tensor num_update_y,
                              int64_t mode) {
        at::AutoDispatchBelowADInplaceOrView below;
        std::pair<at::Tensor, at::Tensor> kept;
        at::Tensor y = adain_impl(x, mean_x, std_x, mean_y, std_y, num_update_x, num_update_y, mode, &kept);
        ctx->save_for_backward({kept.first, kept.second});
        ctx->saved_data["mode"] = mode;
        return y;
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                   torch::autograd::variable_list grads) {
        no_double_backward("adain");
        at::AutoDispatchBelowADInplaceOrView below;
        const auto saved = ctx->get_saved_variables();
        at::Tensor gx = adain_backward_op(grads[0].contiguous(), saved[0], saved[1], ctx->saved_data["mode"].toInt());
        torch::autograd::variable_list out(8);
        out[0] = gx;
        return out;
    }
};

at::Tensor noise_synth_autograd(at::Tensor amp, at::Tensor u, int64_t n_band, int64_t noise_bands) {
    if (at::GradMode::is_enabled() && (amp.requires_grad() || u.requires_grad())) {
        TORCH_CHECK_NOT_IMPLEMENTED(!u.requires_grad(),
                                    "noise_synth: the draw u is a constant; its gradient is not implemented");
        seam_tensor(amp, "amp");
        return NoiseSynthFn::apply(amp, u, n_band, noise_bands);
    }
    at::AutoDispatchBelowADInplaceOrView below;
    return noise_synth_op(amp, u, n_band, noise_bands);
}

at::Tensor adain_autograd(at::Tensor x, at::Tensor mean_x, at::Tensor std_x, at::Tensor mean_y, at::Tensor std_y,
                          at::Tensor num_update_x, at::Tensor num_update_y, int64_t mode) {
    if (at::GradMode::is_enabled() && x.requires_grad()) {
        seam_tensor(x, "x");
        return AdainFn::apply(x, mean_x, std_x, mean_y, std_y, num_update_x, num_update_y, mode);
    }
    at::AutoDispatchBelowADInplaceOrView below;
    return adain_op(x, mean_x, std_x, mean_y, std_y, num_update_x, num_update_y, mode);
}

// rave_amd::delay_line -- cached_conv's CachedPadding1d on rave_copy: returns
// [state[:B] | x] (B, C, P + T), or its first T columns when `crop` (a pure
// P-sample delay), and keeps the newest P columns in `state` (max_batch, C, P).
at::Tensor delay_line_op(at::Tensor x, at::Tensor state, bool crop) {
    seam_tensor(x, "x");
    seam_tensor(state, "state");
    c10::hip::HIPGuard g((c10::DeviceIndex)x.get_device());
    TORCH_CHECK_VALUE(x.dim() == 3 && state.dim() == 3 && state.size(1) == x.size(1) && state.size(0) >= x.size(0) &&
                          state.is_contiguous(),
                      "state must be a contiguous (max_batch, C, P) buffer with x's channels");
    const int64_t B = x.size(0), C = x.size(1), T = x.size(2), P = state.size(2);
    at::Tensor xc = x.contiguous();
    at::Tensor full = at::empty({B, C, P + T}, x.options());
    void* st = cur_stream(x);
    auto copy = [&](const float* src, int64_t s_sb, int64_t s_sc, float* dst, int64_t d_sb, int64_t d_sc, int64_t n) {
        if (n <= 0) return;
        rave_copy_args a{};
        a.batch = (int)B; a.channels = (int)C; a.t_len = (int)n;
        a.x = src; a.x_sb = s_sb; a.x_sc = s_sc;
        a.y = dst; a.y_sb = d_sb; a.y_sc = d_sc;
        check(rave_copy(&a, st), "delay_line");
    };
    float* f = full.data_ptr<float>();
    float* sp = state.data_ptr<float>();
    copy(sp, C * P, P, f, C * (P + T), P + T, P);                                   // history
    copy(xc.data_ptr<float>(), xc.stride(0), xc.stride(1), f + P, C * (P + T), P + T, T);   // block
    copy(f + T, C * (P + T), P + T, sp, C * P, P, P);                               // newest P -> state
    return crop ? full.narrow(2, 0, T) : full;
}

// rave_amd::rvq_encode / rvq_decode -- ResidualVectorQuantization.encode / decode
// (rave/quantization.py:302-318): z (B, D, T), codebooks (n_q, K, D) -> idx (B, n_q, T) int64
at::Tensor rvq_encode_op(at::Tensor z, at::Tensor codebooks) {
    seam_tensor(z, "z");
    c10::hip::HIPGuard g((c10::DeviceIndex)z.get_device());
    at::Tensor cb = codebooks.to(z.device(), at::kFloat).contiguous();
    TORCH_CHECK_VALUE(cb.dim() == 3 && cb.size(2) == z.size(1), "codebooks must be (n_q, K, D)");
    const int64_t B = z.size(0), D = z.size(1), T = z.size(2), nq = cb.size(0);
    at::Tensor idx = at::empty({B, nq, T}, z.options().dtype(at::kLong));
    rave_rvq_args a{};
    a.n_q = (int)nq; a.codebook_size = (int)cb.size(1); a.dim = (int)D; a.batch = (int)B; a.t_len = (int)T;
    a.codebooks = cb.data_ptr<float>();
    a.z = z.data_ptr<float>(); a.z_sb = z.stride(0); a.z_sc = z.stride(1);
    a.idx = idx.data_ptr<int64_t>(); a.i_sb = nq * T; a.i_sq = T;
    const int64_t nw = rave_rvq_workspace(&a);
    if (nw < 0) check((int)nw, "rvq_workspace");
    at::Tensor work = at::empty({std::max<int64_t>(nw, 1)}, z.options());
    a.work = work.data_ptr<float>();
    check(rave_rvq_encode(&a, cur_stream(z)), "rvq_encode");
    return idx;
}

at::Tensor rvq_decode_op(at::Tensor idx, at::Tensor codebooks) {
    TORCH_CHECK_VALUE(idx.is_cuda() && idx.scalar_type() == at::kLong && idx.dim() == 3, "idx must be (B, n_q, T) int64");
    c10::hip::HIPGuard g((c10::DeviceIndex)idx.get_device());
    at::Tensor ic = idx.contiguous();
    at::Tensor cb = codebooks.to(idx.device(), at::kFloat).contiguous();
    TORCH_CHECK_VALUE(cb.dim() == 3 && cb.size(0) == idx.size(1), "codebooks must be (n_q, K, D)");
    const int64_t B = idx.size(0), nq = idx.size(1), T = idx.size(2), D = cb.size(2);
    at::Tensor y = at::empty({B, D, T}, idx.options().dtype(at::kFloat));
    rave_rvq_args a{};
    a.n_q = (int)nq; a.codebook_size = (int)cb.size(1); a.dim = (int)D; a.batch = (int)B; a.t_len = (int)T;
    a.codebooks = cb.data_ptr<float>();
    a.idx = ic.data_ptr<int64_t>(); a.i_sb = nq * T; a.i_sq = T;
    a.y = y.data_ptr<float>(); a.y_sb = D * T; a.y_sc = T;
    check(rave_rvq_decode(&a, cur_stream(idx)), "rvq_decode");
    return y;
}

using State = std::tuple<std::vector<int64_t>, double, std::vector<std::string>, std::vector<at::Tensor>, at::Tensor,
                         int64_t, int64_t>;

}  // namespace

TORCH_LIBRARY(rave_amd, lib) {
    lib.def("fir(Tensor x, Tensor h, int stride, int pad_left, int pad_right, Tensor? hist) -> Tensor", &fir_op);
    lib.def("pack_conv1d(Tensor w, int c_in, int c_out, int kernel, int stride, int dilation, bool transposed, "
            "int out_shift, int precision) -> Tensor", &pack_conv1d_op);
    lib.def("conv1d_packed_size(int c_in, int c_out, int kernel, int stride, int dilation, bool transposed) -> int",
            &conv1d_packed_size_op);
    lib.def("pack_conv1d_device_(Tensor w, Tensor(a!) packed, int c_in, int c_out, int kernel, int stride, int dilation, "
            "bool transposed, int out_shift) -> Tensor(a!)", &pack_conv1d_device_op);
    lib.def("conv1d(Tensor x, Tensor packed, Tensor? bias, Tensor? alpha, Tensor? residual, int c_out, int kernel, "
            "int stride, int dilation, int pad_left, int pad_right, bool transposed, int out_shift, int act, "
            "float slope, int precision) -> Tensor", &conv1d_op);
    lib.def("conv1d_w(Tensor x, Tensor weight, Tensor packed, Tensor? bias, Tensor? alpha, Tensor? residual, int c_out, "
            "int kernel, int stride, int dilation, int pad_left, int pad_right, int act, float slope, int precision) "
            "-> Tensor", &conv1d_w_op);
    lib.def("conv1d_backward(Tensor gy, Tensor? x, Tensor? weight, Tensor? alpha, int c_in, int t_in, int kernel, "
            "int stride, int dilation, "
            "int pad_left, int pad_right, int act, float slope, int need) -> (Tensor? gx, Tensor? gweight, "
            "Tensor? gbias, Tensor? galpha)", &conv1d_backward_op);
    lib.def("conv_transpose1d_w(Tensor x, Tensor weight, Tensor packed, Tensor? bias, Tensor? alpha, Tensor? residual, "
            "int c_out, int kernel, int stride, int act, float slope, int precision) -> Tensor", &conv_transpose1d_w_op);
    lib.def("conv_transpose1d_backward(Tensor gy, Tensor? x, Tensor? weight, Tensor? alpha, int c_in, int t_in, "
            "int kernel, int stride, int act, float slope, int need) -> (Tensor? gx, Tensor? gweight, Tensor? gbias, "
            "Tensor? galpha)", &conv_transpose1d_backward_op);
    lib.def("pqmf_analysis(Tensor x, Tensor hkf, int n_out_bands, int pad_left, int precision) -> Tensor",
            &pqmf_analysis_op);
    lib.def("pqmf_synthesis(Tensor x, Tensor hki, int pad_left, int frames, int frame0, int precision, int mode=0, "
            "Tensor? noise=None) -> Tensor",
            &pqmf_synthesis_op);
    lib.def("pqmf_analysis_backward(Tensor gy, Tensor hkf, int n_out_bands, int pad_left, int t_in) -> Tensor",
            &pqmf_analysis_backward_op);
    lib.def("pqmf_synthesis_backward(Tensor gy, Tensor x, Tensor hki, int pad_left, int frames, int frame0, "
            "int x_len, int mode, Tensor? noise=None) -> (Tensor gx, Tensor? gnoise)",
            &pqmf_synthesis_backward_op);
    lib.def("adain(Tensor x, Tensor(a!) mean_x, Tensor(b!) std_x, Tensor(c!) mean_y, Tensor(d!) std_y, "
            "Tensor(e!) num_update_x, Tensor(f!) num_update_y, int mode) -> Tensor",
            &adain_op);
    lib.def("adain_backward(Tensor gy, Tensor stats, Tensor counters, int mode) -> Tensor", &adain_backward_op);
    lib.def("noise_synth(Tensor amp, Tensor u, int n_band, int noise_bands) -> Tensor", &noise_synth_op);
    lib.def("noise_synth_backward(Tensor gy, Tensor amp, Tensor u, int n_band, int noise_bands) -> Tensor",
            &noise_synth_backward_op);
    lib.def("delay_line(Tensor x, Tensor(a!) state, bool crop) -> Tensor", &delay_line_op);
    lib.def("rvq_encode(Tensor z, Tensor codebooks) -> Tensor", &rvq_encode_op);
    lib.def("rvq_decode(Tensor idx, Tensor codebooks) -> Tensor", &rvq_decode_op);
    lib.class_<Engine>("Engine")
        .def(torch::init<std::vector<int64_t>, double, std::vector<std::string>, std::vector<at::Tensor>, at::Tensor,
                         int64_t, int64_t>())
        .def("encode", &Engine::encode)
        .def("decode", &Engine::decode)
        .def("forward", &Engine::forward)
        .def("encode_codes", &Engine::encode_codes)
        .def("decode_codes", &Engine::decode_codes)
        .def("stream_encode", &Engine::stream_encode)
        .def("stream_decode", &Engine::stream_decode)
        .def("stream_encode_codes", &Engine::stream_encode_codes)
        .def("stream_decode_codes", &Engine::stream_decode_codes)
        .def("stream_reset", &Engine::stream_reset)
        .def("adain_control", &Engine::adain_control)
        .def("set_speaker", &Engine::set_speaker)
        .def("check", &Engine::check_status)
        .def("set_tuning", &Engine::set_tuning)
        .def("hop", &Engine::get_hop)
        .def("latent_channels", &Engine::latent_channels)
        .def("block", &Engine::block)
        .def_pickle(
            [](const c10::intrusive_ptr<Engine>& e) -> State {
                std::vector<at::Tensor> ps;
                for (auto& p : e->params) ps.push_back(p.detach().cpu());
                return State(e->cfg_ints, e->slope, e->names, ps, e->speaker.detach().cpu(), e->precision,
                             e->stream_block);
            },
            [](State st) -> c10::intrusive_ptr<Engine> {
                return c10::make_intrusive<Engine>(std::get<0>(st), std::get<1>(st), std::get<2>(st), std::get<3>(st),
                                                   std::get<4>(st), std::get<5>(st), std::get<6>(st));
            });
}

// A direct registration on the GPU's autograd key: the ops above are defined
// with catch-all kernels, which the dispatcher would otherwise also use there.
TORCH_LIBRARY_IMPL(rave_amd, AutogradCUDA, m) {
    m.impl("pqmf_analysis", &pqmf_analysis_autograd);
    m.impl("pqmf_synthesis", &pqmf_synthesis_autograd);
    m.impl("conv1d_w", &conv1d_w_autograd);
    m.impl("conv_transpose1d_w", &conv_transpose1d_w_autograd);
    m.impl("adain", &adain_autograd);
    m.impl("noise_synth", &noise_synth_autograd);
}
