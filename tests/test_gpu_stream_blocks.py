"""Streaming at every block length against the float64 cached-mode model
(tests/stream_ref.py, pinned on the CPU by tests/test_stream_ref_host.py).  Runs
on an MI355X only (``-m gpu``).

The stream plan (rave_amd/csrc/engine.cpp: build_stream, stream_buffers,
conv_stream, stream_convs, shift_all, direct_input) depends on the block
length at every step -- the history offset of every buffer, whether the fp32
ring kernels' 16-byte rows apply, which units fuse, the skinny-N tiles, the
noise frame count, the synthesis shift, the graph mode's direct input copy --
and the other streaming tests run it at 2048 samples.  Here every config of
``sweep_configs`` (capacity 8; hop 1024 with dilations up to 9, and a hop-64 /
hop-256 pair whose block is shorter than the PQMF histories) streams one
B = 2 signal in blocks of 1, 2, 3, 4, 5, 7, 8 (and 17) latent frames, graph
and eager, and is compared from sample 0 with ONE evaluation of the reference:
the cached mode does not depend on the partition (test_partition_invariance).
The same reference bounds the operator seam (``cc`` under use_cached_conv, fed
blocks whose length changes from call to call) and, through the offline
oracle, the one-shot engine at clips of 1 to 24 frames.

Bounds.  split16 and auto: the project's 1e-4.  The exact-fp32 classes (f32,
f32_tuned, f32_bf3): K * e32, never above 1e-4, where e32 is the max-abs error
of the reference itself run in float32 on the same signal (computed here, from
the reference only) and K is the next power of two above the worst kernel
error / e32 measured on an MI355X over every case of this file, one K per
direction (the GPU and numpy sum in different orders, so a ratio of a few is
expected):

    K_ENC = 1: worst encode ratio 0.86 (causal_hop64, 17-frame blocks and the
               24-frame one-shot clip, f32; the other configs reach 0.55 to 0.74)
    K_DEC = 4: worst decode ratio 2.89 (v3_noise, 8-frame blocks, f32_bf3; f32
               reaches 2.72 there; the other configs reach 1.72 to 2.39)

The ratios of split16 and auto on the same cases stay below 1.5 e32.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.stream_ref import (StreamRef, noise_frames_per_latent, run_stream, sweep_configs,  # noqa: E402
                              sweep_signals)

pytestmark = pytest.mark.gpu

TOL = 1e-4
K_ENC = 1.0
K_DEC = 4.0
EXACT = ("f32", "f32_tuned", "f32_bf3")
HOP1024 = ["causal", "v2", "v3_noise_causal", "v3_noise", "discrete"]
SHORT = ["causal_hop64", "v3_noise_causal_hop256"]
LENGTHS = [(n, k) for n in HOP1024 + SHORT for k in (1, 2, 3, 4, 5, 7, 8) + ((17,) if n in SHORT else ())]
SEED = 0


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hk(golden):
    return golden("pqmf")["hk"]


# ------------------------------------------------------------------ the reference, once per signal
_CASES = {}


def _case(name, hk, batch=2):
    """Config, signal, and the float64 cached model's outputs for it (one
    evaluation: any partition gives them), with e32 per direction."""
    key = (name, batch)
    if key in _CASES:
        return _CASES[key]
    from rave_amd.weights import init_params, init_speaker
    cfg, frames = sweep_configs()[name]
    c = {"name": name, "cfg": cfg, "frames": frames, "B": batch, "params": init_params(cfg, SEED),
         "spk": init_speaker(cfg, SEED), "sig": sweep_signals(cfg, frames, batch)}
    out = {}
    for dt in (np.float64, np.float32):
        r = StreamRef(cfg, c["params"], c["spk"], hk=hk, dtype=dt)
        o = {"z": run_stream(r, c["sig"], [frames], "encode")}
        if cfg.rvq is not None:
            r.reset()
            o["idx"], o["gap"] = run_stream(r, c["sig"], [frames], "encode_codes")
            if dt == np.float64:
                c["sig"]["z"] = np.asarray(r.cat_speaker(r.rvq_decode(o["idx"])), np.float32)   # what the codes decode to
                c["idx"], c["gap"] = o["idx"], o["gap"].transpose(1, 0, 2)                       # gap: (B, n_q, frames)
            # both precisions decode the float64 model's codes
            o["y"] = r.decode_codes(c["idx"])
        else:
            o["y"] = run_stream(r, c["sig"], [frames], "decode")
        out[dt] = o
    c["z"], c["y"] = out[np.float64]["z"], out[np.float64]["y"]
    c["e32_z"], c["e32_y"] = maxabs(out[np.float32]["z"], c["z"]), maxabs(out[np.float32]["y"], c["y"])
    assert np.isfinite(c["z"]).all() and np.isfinite(c["y"]).all() and c["e32_z"] > 0 and c["e32_y"] > 0
    _CASES[key] = c
    return c


def _tols(c, precision):
    if precision in EXACT:
        return min(K_ENC * c["e32_z"], TOL), min(K_DEC * c["e32_y"], TOL)
    return TOL, TOL


_MODELS = {}


def _model(c, dev, hk, precision="f32"):
    """One engine model per (config, precision), kept for the module's tests of it
    (only the latest few: each holds device memory)."""
    from rave_amd.model import RAVE
    key = (c["name"], precision)
    if key not in _MODELS:
        while len(_MODELS) >= 3:
            _MODELS.pop(next(iter(_MODELS)))
        _MODELS[key] = RAVE(c["cfg"], c["params"], c["spk"], device=dev, hk=hk, precision=precision)
    return _MODELS[key]


def _noise(c, dev, a, b):
    """The uniform draws of latent frames [a, b) (None without a noise synthesizer)."""
    if c["cfg"].noise is None:
        return None
    per = noise_frames_per_latent(c["cfg"])
    return torch.from_numpy(np.ascontiguousarray(c["sig"]["u"][:, a * per:b * per])).to(dev)


def _tensors(c, dev):
    if "dev" not in c:
        c["dev"] = {"x": torch.from_numpy(c["sig"]["x"]).to(dev), "z": torch.from_numpy(c["sig"]["z"]).to(dev)}
        if c["cfg"].rvq is not None:
            c["dev"]["idx"] = torch.from_numpy(c["idx"]).to(dev)
    return c["dev"]


def _enc_block(s, c, dev, i, k):
    """Block i of k frames through the stream's encoder: latents, or indices for a discrete config."""
    hop = c["cfg"].hop
    x = _tensors(c, dev)["x"][..., i * k * hop:(i + 1) * k * hop].contiguous()
    return s.encode_codes(x) if c["cfg"].rvq is not None else s.encode(x)


def _dec_block(s, c, dev, i, k):
    u = _noise(c, dev, i * k, (i + 1) * k)
    if c["cfg"].rvq is not None:
        return s.decode_codes(_tensors(c, dev)["idx"][..., i * k:(i + 1) * k].contiguous(), noise_u=u)
    return s.decode(_tensors(c, dev)["z"][..., i * k:(i + 1) * k].contiguous(), noise_u=u)


def _check(c, precision, enc, dec, n, tag):
    """Streamed outputs over the first n frames against the reference; returns
    the error / e32 ratios (encode, decode).  Latents: every channel, the
    speaker's included (bitwise there).  Discrete: indices outside the tie
    margin."""
    cfg = c["cfg"]
    tz, ty = _tols(c, precision)
    assert torch.isfinite(dec).all()
    ey = maxabs(dec.cpu().numpy(), c["y"][..., :n * cfg.hop])
    if cfg.rvq is not None:
        got = enc.cpu().numpy()
        mism = got != c["idx"][..., :n]
        worst_gap = float(c["gap"][..., :n][mism].max()) if mism.any() else 0.0
        print(f"\n[blocks] {tag} {precision}: {int(mism.sum())} index mismatches (worst gap {worst_gap:.1e}), "
              f"y {ey:.3e} = {ey / c['e32_y']:.2f} e32 (bound {ty:.2e})")
        assert worst_gap < 1e-3, tag
        assert ey < ty, tag
        return 0.0, ey / c["e32_y"]
    assert torch.isfinite(enc).all()
    z = enc.cpu().numpy()
    ez = maxabs(z, c["z"][..., :n])
    print(f"\n[blocks] {tag} {precision}: z {ez:.3e} = {ez / c['e32_z']:.2f} e32 (bound {tz:.2e}), "
          f"y {ey:.3e} = {ey / c['e32_y']:.2f} e32 (bound {ty:.2e})")
    spk = np.broadcast_to(np.asarray(c["spk"], np.float32).reshape(1, -1, 1), z[:, cfg.latent_size:].shape)
    assert np.array_equal(z[:, cfg.latent_size:], spk), tag      # fill_speaker / the staged fill
    assert ez < tz and ey < ty, tag
    return ez / c["e32_z"], ey / c["e32_y"]


# ------------------------------------------------------------------ every block length, graph and eager, f32
_SEEN = {}


@pytest.mark.parametrize("name,k", LENGTHS)
def test_stream_block_lengths_f32(dev, hk, name, k):
    """Blocks of k latent frames, a graph stream and an eager one side by side:
    bitwise equal at every block (the graph's direct input copy lands at a
    history offset that is no multiple of 4 floats at most of these lengths)
    and after a reset(); the first block after the reset is the first block of
    the fresh stream, bitwise; both within the bound of the reference from
    sample 0; ``decode_delay`` is the reference's."""
    from rave_amd.streaming import StreamingRAVE
    c = _case(name, hk)
    m = _model(c, dev, hk)
    sg = StreamingRAVE(m, batch=c["B"], block=k * c["cfg"].hop, graph=True)
    se = StreamingRAVE(m, batch=c["B"], block=k * c["cfg"].hop, graph=False)
    ref = StreamRef(c["cfg"], {}, c["spk"], hk=hk)
    assert sg.decode_delay == se.decode_delay == ref.decode_delay()
    nb = c["frames"] // k
    enc, dec = [], []
    for i in range(nb):
        zg, ze = _enc_block(sg, c, dev, i, k), _enc_block(se, c, dev, i, k)
        yg, ye = _dec_block(sg, c, dev, i, k), _dec_block(se, c, dev, i, k)
        torch.cuda.synchronize()
        assert torch.equal(zg, ze) and torch.equal(yg, ye), (name, k, i)
        enc.append(zg)
        dec.append(yg)
    for s in (sg, se):
        s.reset()
        z0, y0 = _enc_block(s, c, dev, 0, k), _dec_block(s, c, dev, 0, k)
        torch.cuda.synchronize()
        assert torch.equal(z0, enc[0]) and torch.equal(y0, dec[0]), (name, k)
    enc, dec = torch.cat(enc, -1), torch.cat(dec, -1)
    _check(c, "f32", enc, dec, nb * k, f"{name} k={k}")
    # partitions against each other (the reference bounds each; this is a figure)
    seen = _SEEN.setdefault(name, {})
    seen[k] = (enc.float().cpu().numpy(), dec.cpu().numpy())
    n = min(v[1].shape[-1] for v in seen.values())
    worst = max([maxabs(a[1][..., :n], b[1][..., :n]) for a in seen.values() for b in seen.values()])
    print(f"[blocks] {name}: worst pairwise decode difference between block lengths {sorted(seen)}: {worst:.3e}")


# ------------------------------------------------------------------ the other precisions
@pytest.mark.parametrize("precision", ["split16", "auto", "f32_bf3"])
@pytest.mark.parametrize("name", HOP1024 + SHORT)
def test_stream_block_lengths_other_precisions(dev, hk, name, precision):
    """Blocks of 1, 3 and 8 frames in the other arithmetic classes."""
    _other_precision(dev, hk, name, precision)


def test_stream_block_lengths_f32_tuned(dev, hk):
    """f32_tuned (exact fp32 with the ring kernels, timed at plan build) in one config."""
    _other_precision(dev, hk, "causal", "f32_tuned")


def _other_precision(dev, hk, name, precision):
    from rave_amd.streaming import StreamingRAVE
    c = _case(name, hk)
    m = _model(c, dev, hk, precision)
    for k in (1, 3, 8):
        s = StreamingRAVE(m, batch=c["B"], block=k * c["cfg"].hop)
        nb = c["frames"] // k
        enc = torch.cat([_enc_block(s, c, dev, i, k) for i in range(nb)], -1)
        dec = torch.cat([_dec_block(s, c, dev, i, k) for i in range(nb)], -1)
        torch.cuda.synchronize()
        _check(c, precision, enc, dec, nb * k, f"{name} k={k}")


# ------------------------------------------------------------------ two streams on one model; B = 3
@pytest.mark.parametrize("name", ["v2", "v3_noise_causal_hop256"])
def test_two_streams_of_different_block_lengths(dev, hk, name):
    """Two streams of different block lengths alive on one model, fed
    alternately: each still matches the reference."""
    from rave_amd.streaming import StreamingRAVE
    c = _case(name, hk)
    m = _model(c, dev, hk)
    ks = (2, 3)
    ss = [StreamingRAVE(m, batch=c["B"], block=k * c["cfg"].hop) for k in ks]
    outs = [([], []) for _ in ks]
    for i in range(c["frames"] // min(ks)):
        for s, k, (enc, dec) in zip(ss, ks, outs):
            if (i + 1) * k <= c["frames"]:
                enc.append(_enc_block(s, c, dev, i, k))
                dec.append(_dec_block(s, c, dev, i, k))
    torch.cuda.synchronize()
    for k, (enc, dec) in zip(ks, outs):
        _check(c, "f32", torch.cat(enc, -1), torch.cat(dec, -1), len(enc) * k, f"{name} k={k} interleaved")


def test_batch_of_three(dev, hk):
    """B = 3 (an odd batch stride), blocks of 3 frames, centred v2."""
    from rave_amd.streaming import StreamingRAVE
    c = _case("v2", hk, batch=3)
    m = _model(c, dev, hk)
    k = 3
    s = StreamingRAVE(m, batch=3, block=k * c["cfg"].hop)
    nb = c["frames"] // k
    enc = torch.cat([_enc_block(s, c, dev, i, k) for i in range(nb)], -1)
    dec = torch.cat([_dec_block(s, c, dev, i, k) for i in range(nb)], -1)
    torch.cuda.synchronize()
    assert maxabs(c["y"][0], c["y"][2]) > 1e-3
    _check(c, "f32", enc, dec, nb * k, "v2 B=3 k=3")


# ------------------------------------------------------------------ the operator seam
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", ["causal", "v2"])
def test_cc_cached_tree_changing_block_lengths(dev, hk, name, batch):
    """The ``cc`` module tree built under use_cached_conv(True), fed blocks of
    1, 3, 2, 5, 1, 8 frames in turn (its delay lines take any length; the
    engine's plans cannot), against the same reference with the same bound."""
    from rave_amd import cc
    from rave_amd.modules import RAVEModules, load_reference_state
    c = _case(name, hk)
    cc.use_cached_conv(True)
    cc.set_precision("f32")
    try:
        m = RAVEModules(c["cfg"], c["spk"], hk=hk)
    finally:
        cc.use_cached_conv(False)
    load_reference_state(m, c["params"])
    m = m.to(dev).eval()
    t = _tensors(c, dev)
    hop = c["cfg"].hop
    enc, dec, pos = [], [], 0
    with torch.no_grad():
        for k in (1, 3, 2, 5, 1, 8):
            enc.append(m.encode(t["x"][:batch, :, pos * hop:(pos + k) * hop]))
            dec.append(m.decode(t["z"][:batch, :, pos:pos + k]))
            pos += k
    torch.cuda.synchronize()
    sub = dict(c, z=c["z"][:batch], y=c["y"][:batch])      # the batch rows are independent
    _check(sub, "f32", torch.cat(enc, -1), torch.cat(dec, -1), pos, f"cc tree {name} B={batch} blocks 1,3,2,5,1,8")


# ------------------------------------------------------------------ the one-shot engine at short clips
_ONESHOT = {}


@pytest.mark.parametrize("frames", [1, 2, 3, 5, 24])
@pytest.mark.parametrize("name", HOP1024 + SHORT)
def test_oneshot_short_clips(dev, hk, name, frames):
    """m.encode / m.decode of the first 1, 2, 3, 5 and 24 latent frames of the
    same signals against the offline oracle (the other model tests start at
    16384 samples), within the same bounds."""
    from oracle.rave_oracle import Oracle
    c = _case(name, hk)
    cfg = c["cfg"]
    m = _model(c, dev, hk)
    o = Oracle(cfg, c["params"], c["spk"], hk=hk)
    t = _tensors(c, dev)
    x, z = c["sig"]["x"][..., :frames * cfg.hop], c["sig"]["z"][..., :frames]
    per = noise_frames_per_latent(cfg) if cfg.noise is not None else 0
    u = c["sig"]["u"][:, :frames * per] if cfg.noise is not None else None
    ref = dict(c, z=o.encode(x), y=o.decode(z, u))
    if cfg.rvq is not None:
        ref["idx"], gap = o.rvq_encode(ref["z"], return_gaps=True)
        ref["gap"] = gap.reshape(gap.shape[0], c["B"], frames).transpose(1, 0, 2)
        enc = m.encode_codes(t["x"][..., :frames * cfg.hop].contiguous())
        # the clip's own codes need not be the stream's: decode the stream's, as the reference y does
        dec = m.decode_codes(t["idx"][..., :frames].contiguous(), noise_u=_noise(c, dev, 0, frames))
    else:
        enc = m.encode(t["x"][..., :frames * cfg.hop].contiguous())
        dec = m.decode(t["z"][..., :frames].contiguous(), noise_u=_noise(c, dev, 0, frames))
    torch.cuda.synchronize()
    _check(ref, "f32", enc, dec, frames, f"one-shot {name} {frames} frames")
