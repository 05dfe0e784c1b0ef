"""Per-row target speakers on the GPU: a model's speaker table, the two modes
(shared / per-row) and every site that writes speaker channels -- the fill op,
the fill fused into the encoder head, the fill after rvq.decode -- through
encode, forward, decode_codes, the streaming engine, convert and validate.

Embeddings are distinct per row (row r ~ N(0, 1), seed 100 + r), so a wrong
row index cannot pass.  The oracle results are computed once per config and
shared (oracle latent of the batch, decoded with each row's own embedding).

Bars: 1e-4 max-abs against the float64 oracle on audio (the project's standing
parity bar), 1e-4 relative on the distance (tests/test_gpu_distance.py's), and
bitwise wherever two runs of this engine execute the same plan on the same
row: batch is a grid dimension of every kernel, so row b of a batch depends on
row b's inputs alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
S = 256                       # speaker_size of every config here
B3, T4 = 3, 4096              # 4 latent frames at hop 1024


def emb(r):
    return np.random.default_rng(100 + r).standard_normal(S).astype(np.float32)


def embs(*rows):
    return np.stack([emb(r) for r in rows])


def audio(B, T, seed=7):
    n = np.arange(T)
    rng = np.random.default_rng(seed)
    x = np.stack([0.3 * np.sin(2 * np.pi * (220.0 * (b + 1)) * n / 48000) for b in range(B)])
    return (x + 0.1 * rng.standard_normal((B, T))).astype(np.float32)[:, None]


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _params(cfg, seed=0):
    from rave_amd.weights import init_params, init_speaker
    return init_params(cfg, seed=seed), init_speaker(cfg, seed=seed)


def _model(cfg, seed=0, **kw):
    from rave_amd.model import RAVE
    p, spk = _params(cfg, seed)
    return RAVE(cfg, p, spk, device=DEV, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_rows(name):
    """(x, E, oracle latent, oracle audio): row b decoded from
    cat(oracle latent[b], E[b]).  Computed once per config."""
    from oracle.rave_oracle import Oracle
    from rave_amd import config as rcfg
    from rave_amd import pqmf as P
    cfg = rcfg.get_config(name)
    p, spk = _params(cfg)
    x = audio(B3, T4)
    E = embs(0, 1, 2)
    o = Oracle(cfg, p, spk, hk=P.design_bank(cfg.pqmf_attenuation, cfg.n_band))
    lat = np.asarray(o.encode(x))[:, :cfg.latent_size]
    z = np.concatenate([lat, np.broadcast_to(E[:, :, None].astype(np.float64), (B3, S, lat.shape[-1]))], 1)
    y = np.asarray(o.decode(z))
    for v in (x, E, lat, y):
        v.setflags(write=False)
    return x, E, lat, y


# ------------------------------------------------------------------ 1. raw fill
def test_raw_fill_row_stride():
    """rave_fill_channels at (B 3, C 5, T 7) into a non-contiguous view with
    guard elements around it: with a row stride y[b] = values[b] broadcast,
    with stride 0 today's result, both exactly; nothing else is written."""
    from rave_amd import _native as N
    B, Cc, T = 3, 5, 7
    rng = np.random.default_rng(1)
    SENT = -12345.0
    vs = Cc + 3                                                   # rows wider than the channels used
    vals = torch.from_numpy(rng.standard_normal((B, vs)).astype(np.float32)).to(DEV)
    v0 = vals.clone()
    for stride in (vs, 0):
        buf = torch.full((B + 2, Cc + 3, T + 5), SENT, device=DEV)
        y = buf[1:1 + B, 2:2 + Cc, 3:3 + T]                       # y_sb, y_sc != C*T, T
        assert y.stride(0) != Cc * T and y.stride(1) != T
        a = N.FillArgs(batch=B, channels=Cc, t_len=T, values_sb=stride, y=y.data_ptr(), y_sb=y.stride(0),
                       y_sc=y.stride(1), values=vals.data_ptr())
        N.check(N.lib.rave_fill_channels(C.byref(a), _st()))
        torch.cuda.synchronize()
        want = (vals[:, :Cc] if stride else vals[:1, :Cc].expand(B, Cc))[:, :, None].expand(B, Cc, T)
        assert torch.equal(y, want), stride
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[1:1 + B, 2:2 + Cc, 3:3 + T] = False
        assert bool((buf[mask] == SENT).all()), stride
        assert torch.equal(vals, v0)
    # stride 0 is what a caller that never heard of the field passes
    assert N.FillArgs(batch=B, channels=Cc, t_len=T).values_sb == 0


# ------------------------------------------------------------------ 2. encode
@pytest.mark.parametrize("site,precision", [("head", "split16"), ("fill", "f32")])
def test_encode_reads_its_table_rows(site, precision):
    """v2, B 3, 4 frames, a 4-row table read from row 1: the speaker channels
    of z[b] are table row 1 + b exactly, the latent channels are bitwise those
    of a shared-mode encode.  split16 runs the fill fused into the encoder
    head, f32 the separate fill op (asserted on the plan's op list)."""
    from rave_amd import _native as N
    from rave_amd import config as rcfg
    from rave_amd.model import ENCODE
    cfg = rcfg.v2()
    m = _model(cfg, precision=precision, speaker_rows=4)
    assert m.speaker_rows == 4 and m.speaker_row0 == 0 and not m.per_row_speakers
    kinds = [o["kind"] for o in m.ops(ENCODE, B3, T4)]
    assert (N.OP_HEAD in kinds, N.OP_FILL in kinds) == ((True, False) if site == "head" else (False, True))
    x = torch.from_numpy(audio(B3, T4)).to(DEV)
    lat = cfg.latent_size
    z_sh = m.encode(x).clone()
    shared = torch.from_numpy(_params(cfg)[1]).to(DEV)
    assert torch.equal(z_sh[:, lat:], shared[None, :, None].expand(B3, S, 4))
    E = torch.from_numpy(embs(10, 11, 12, 13)).to(DEV)
    m.set_speaker(E)
    m.speaker_row0 = 1
    assert m.per_row_speakers and m.speaker_row0 == 1
    z = m.encode(x)
    torch.cuda.synchronize()
    assert torch.equal(z[:, lat:], E[1:4, :, None].expand(B3, S, 4))
    assert torch.equal(z[:, :lat], z_sh[:, :lat])
    # a partial update reaches its row only; a 1-D vector returns to shared mode
    m.set_speaker(emb(20)[None], row0=2)
    z2 = m.encode(x)
    assert torch.equal(z2[:, lat:][0], E[1, :, None].expand(S, 4))
    assert torch.equal(z2[:, lat:][1], torch.from_numpy(emb(20)).to(DEV)[:, None].expand(S, 4))
    assert torch.equal(z2[:, lat:][2], E[3, :, None].expand(S, 4))
    m.set_speaker(_params(cfg)[1])
    assert not m.per_row_speakers
    assert torch.equal(m.encode(x), z_sh)


# ------------------------------------------------------------------ 3. forward vs the oracle
@pytest.mark.parametrize("precision", ["f32", "f32_bf3"])
@pytest.mark.parametrize("name", ["v2", "causal"])
def test_forward_matches_oracle_per_row(name, precision):
    from rave_amd import config as rcfg
    x, E, lat, want = _oracle_rows(name)
    cfg = rcfg.get_config(name)
    m = _model(cfg, precision=precision)
    m.set_speaker(E)
    xd = torch.from_numpy(x).to(DEV)
    z = m.encode(xd)
    y = m.forward(xd)
    torch.cuda.synchronize()
    assert torch.equal(z[:, cfg.latent_size:].cpu(), torch.from_numpy(E)[:, :, None].expand(B3, S, 4))
    for b in range(B3):
        err = maxabs(y[b].cpu().numpy(), want[b])
        print(f"forward {name} {precision} row {b}: max-abs vs oracle {err:.3e}")
        assert err <= TOL, (b, err)


# ------------------------------------------------------------------ 4. row consistency
def test_per_row_equals_shared_runs_bitwise():
    """Row b of the per-row forward equals row b of a shared-mode forward of the
    same batch with speaker b, bitwise, under one replayed tuning (so both
    models run the same plans)."""
    from rave_amd import config as rcfg
    cfg = rcfg.v2()
    x = torch.from_numpy(audio(B3, T4)).to(DEV)
    E = embs(0, 1, 2)
    m = _model(cfg, precision="f32_bf3")
    m.set_speaker(E)
    y = m.forward(x).clone()
    ref = _model(cfg, precision="f32_bf3", tuning=m.tuning())
    for b in range(B3):
        ref.set_speaker(E[b])
        yb = ref.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(yb[b], y[b]), b
        if b:
            assert not torch.equal(yb[0], y[0])          # the speaker matters at all


# ------------------------------------------------------------------ 5. discrete
def test_decode_codes_per_row():
    """B 2 on fixed indices: each row matches the oracle's rvq.decode -> cat its
    own embedding -> decode."""
    from oracle.rave_oracle import Oracle
    from rave_amd import config as rcfg
    cfg = rcfg.discrete()
    p, spk = _params(cfg)
    m = _model(cfg)
    Fz = 4
    idx = np.random.default_rng(5).integers(0, cfg.rvq.codebook_size, (2, cfg.rvq.num_quantizers, Fz))
    E = embs(0, 1)
    m.set_speaker(E)
    y = m.decode_codes(torch.from_numpy(idx).to(DEV)).cpu().numpy()
    o = Oracle(cfg, p, spk, hk=m.hk)
    q = np.asarray(o.rvq_decode(idx))
    z = np.concatenate([q, np.broadcast_to(E[:, :, None].astype(np.float64), (2, S, Fz))], 1)
    want = np.asarray(o.decode(z))
    for b in range(2):
        err = maxabs(y[b], want[b])
        print(f"decode_codes row {b}: max-abs vs oracle {err:.3e}")
        assert err <= TOL, (b, err)


# ------------------------------------------------------------------ 6. streaming
@pytest.mark.parametrize("graph", [True, False])
def test_stream_rows_follow_their_speakers(graph):
    """Causal, B 3, block 2048.  The per-row stream starts with table (A, B, C),
    gets row 1 = D after block 2, goes to shared A for a block and back to the
    table for one more.  Row b must equal, bitwise, row b of a stream of the
    same batch that ran the matching sequence of shared speakers (the existing
    capability, the same plan)."""
    from rave_amd import config as rcfg
    from rave_amd.streaming import StreamingRAVE
    cfg = rcfg.causal(capacity=8)
    A, Bv, Cv, D = (emb(r) for r in range(4))
    gen = torch.Generator().manual_seed(6)
    xs = [(0.3 * torch.randn(B3, 1, 2048, generator=gen)).to(DEV) for _ in range(6)]

    def run(setter):
        m = _model(cfg, seed=21)
        s = StreamingRAVE(m, batch=B3, block=2048, graph=graph)
        zs, ys = [], []
        for i, x in enumerate(xs):
            setter(s, i)
            z = s.encode(x)
            zs.append(z.clone())
            ys.append(s.decode(z).clone())
        torch.cuda.synchronize()
        return zs, ys

    def per_row(s, i):
        if i == 0:
            s.set_speaker(np.stack([A, Bv, Cv]))
        elif i == 2:
            s.set_speaker(D[None], row0=1)
        elif i == 4:
            s.set_speaker(A)                       # shared
        elif i == 5:
            s.set_speaker(np.stack([A, D, Cv]))    # and back

    def shared(seq):
        def setter(s, i):
            if i in seq:
                s.set_speaker(seq[i])
        return setter

    zs, ys = run(per_row)
    refs = [run(shared({0: A})),
            run(shared({0: Bv, 2: D, 4: A, 5: D})),
            run(shared({0: Cv, 4: A, 5: Cv}))]
    for b, (rz, ry) in enumerate(refs):
        for i in range(len(xs)):
            assert torch.equal(zs[i][b], rz[i][b]), (b, i)
            assert torch.equal(ys[i][b], ry[i][b]), (b, i)
    lat = cfg.latent_size
    assert torch.equal(zs[3][1, lat:, 0].cpu(), torch.from_numpy(D))
    assert torch.equal(zs[4][1, lat:, 0].cpu(), torch.from_numpy(A))
    assert torch.equal(zs[5][2, lat:, 0].cpu(), torch.from_numpy(Cv))


@pytest.mark.parametrize("graph", [True, False])
def test_discrete_stream_decode_follows_a_mode_change(graph):
    """A discrete stream's decoder fills the speaker channels after rvq.decode
    inside its plan, so in graph mode the fill is part of the captured graph: a
    shared <-> per-row switch must re-capture it, a table update must not need to.
    B 2 on fixed indices; rows against streams that ran the shared speakers."""
    from rave_amd import config as rcfg
    from rave_amd.streaming import StreamingRAVE
    cfg = rcfg.discrete(capacity=8)
    A, Bv, D = emb(0), emb(1), emb(3)
    rng = np.random.default_rng(9)
    idx = [torch.from_numpy(rng.integers(0, cfg.rvq.codebook_size, (2, cfg.rvq.num_quantizers, 2))).to(DEV)
           for _ in range(5)]

    def run(seq):
        m = _model(cfg, seed=22)
        s = StreamingRAVE(m, batch=2, block=2 * cfg.hop, graph=graph, direction="decode")
        ys = []
        for i, ix in enumerate(idx):
            if i in seq:
                s.set_speaker(*seq[i])
            ys.append(s.decode_codes(ix).clone())
        torch.cuda.synchronize()
        return ys

    ys = run({0: (A,), 1: (np.stack([A, Bv]),), 2: (D[None], 1), 3: (Bv,), 4: (np.stack([D, A]),)})
    r0 = run({0: (A,), 3: (Bv,), 4: (D,)})
    r1 = run({0: (A,), 1: (Bv,), 2: (D,), 3: (Bv,), 4: (A,)})
    for i in range(len(idx)):
        assert torch.equal(ys[i][0], r0[i][0]), i
        assert torch.equal(ys[i][1], r1[i][1]), i
    assert not torch.equal(r0[2][1], r1[2][1])               # the speaker reaches the audio


# ------------------------------------------------------------------ 7. device hand-off
@pytest.fixture(scope="module")
def handoff():
    from rave_amd import config as rcfg
    from rave_amd.speaker import SpeakerRAVE, init_params as sp_params
    cfg = rcfg.v2()
    m = _model(cfg, precision="f32_bf3")
    spk = SpeakerRAVE(sp_params(0), device=DEV)
    x = torch.from_numpy(audio(B3, T4)).to(DEV)
    return cfg, m, spk, x


def test_set_speaker_takes_the_embedder_output(handoff):
    cfg, m, spk, x = handoff
    e = spk.embed(x)
    assert tuple(e.shape) == (B3, S) and e.device.type == "cuda" and e.dtype == torch.float32
    m.set_speaker(e)
    z = m.encode(x)
    assert torch.equal(z[:, cfg.latent_size:], e[:, :, None].expand(B3, S, 4))


def test_convert_equals_forward_with_permuted_rows(handoff):
    cfg, m, spk, x = handoff
    perm = [1, 2, 0]
    y = m.convert(x, (spk, x[perm])).clone()
    m.set_speaker(spk.embed(x)[perm].contiguous())
    assert torch.equal(m.forward(x), y)
    y2 = m.convert(x, spk.embed(x)[perm])                   # the embeddings form
    assert torch.equal(y2, y)
    m.set_speaker(spk.embed(x))
    assert not torch.equal(m.forward(x), y)


def test_validate_with_a_speaker_encoder(handoff):
    """validate(x, speaker_encoder=spk): each clip decoded with its own
    embedding; the expected distance is composed from per-row oracle outputs
    and the float64 reference distance."""
    from oracle.rave_oracle import Oracle
    from tests.distance_ref import DEFAULT_SCALES, distance
    cfg, m, spk, x = handoff
    got = m.validate(x, speaker_encoder=spk)["spectral_distance"]
    assert got.dim() == 0 and got.device.type == "cuda" and m.per_row_speakers
    E = spk.embed(x).cpu().numpy()
    xn = x.cpu().numpy()
    p, s0 = _params(cfg)
    o = Oracle(cfg, p, s0, hk=m.hk)
    lat = np.asarray(o.encode(xn))[:, :cfg.latent_size]
    z = np.concatenate([lat, np.broadcast_to(E[:, :, None].astype(np.float64), (B3, S, lat.shape[-1]))], 1)
    y = np.asarray(o.decode(z), np.float64)
    x_rt = np.asarray(o.pqmf_synthesis(o.pqmf_analysis(xn)), np.float64)
    want = distance(torch.from_numpy(x_rt), torch.from_numpy(y), DEFAULT_SCALES, 1e-7)
    rel = abs(float(got) - want) / abs(want)
    print(f"validate per-row: got {float(got):.9g} want {want:.9g} rel {rel:.2e}")
    assert rel <= 1e-4


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_everything_untouched():
    from rave_amd import _native as N
    from rave_amd import config as rcfg
    cfg = rcfg.v2(capacity=8)
    m = _model(cfg, speaker_rows=4)
    T = 1024
    E = torch.from_numpy(embs(0, 1, 2, 3)).to(DEV)
    m.set_speaker(E)
    x4 = torch.from_numpy(audio(4, T)).to(DEV)
    z_ok = m.encode(x4).clone()
    SENT = -777.0
    # B = 5 with a 4-row table: RAVE_ERR_ARG before any launch, outputs untouched
    x5 = torch.from_numpy(audio(5, T)).to(DEV)
    z = torch.full((5, cfg.latent_size + S, 1), SENT, device=DEV)
    y = torch.full((5, 1, T), SENT, device=DEV)
    assert N.lib.rave_model_encode(m.handle, x5.data_ptr(), 5, T, z.data_ptr(), _st()) == N.RAVE_ERR_ARG
    assert b"speaker table" in N.lib.rave_last_error()
    assert N.lib.rave_model_forward(m.handle, x5.data_ptr(), 5, T, y.data_ptr(), None, _st()) == N.RAVE_ERR_ARG
    torch.cuda.synchronize()
    assert bool((z == SENT).all()) and bool((y == SENT).all())
    with pytest.raises(ValueError):
        m.encode(x5)
    # the same batch of 4 from row 1 runs past the end, too
    m.speaker_row0 = 1
    z4 = torch.full((4, cfg.latent_size + S, 1), SENT, device=DEV)
    assert N.lib.rave_model_encode(m.handle, x4.data_ptr(), 4, T, z4.data_ptr(), _st()) == N.RAVE_ERR_ARG
    torch.cuda.synchronize()
    assert bool((z4 == SENT).all())
    m.speaker_row0 = 0
    # row0 past the end, as a property and as an update
    with pytest.raises(ValueError):
        m.speaker_row0 = 4
    assert m.speaker_row0 == 0
    with pytest.raises(ValueError):
        m.set_speaker(E[:2], row0=3)
    assert N.lib.rave_model_set_speakers(m.handle, E.data_ptr(), 2, 3, _st()) == N.RAVE_ERR_ARG
    assert N.lib.rave_model_set_speakers(m.handle, E.data_ptr(), 1, 4, _st()) == N.RAVE_ERR_ARG
    assert N.lib.rave_model_set_speakers(m.handle, E.data_ptr(), 0, 0, _st()) == N.RAVE_ERR_ARG
    # wrong width, and a device tensor that is not float32
    with pytest.raises(ValueError):
        m.set_speaker(torch.zeros(2, S - 1, device=DEV))
    with pytest.raises(ValueError):
        m.set_speaker(torch.zeros(2, S, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        m.set_speaker(torch.zeros(2, S, device=DEV, dtype=torch.float16))
    # none of it changed the table, the mode or row0
    assert m.per_row_speakers
    assert torch.equal(m.encode(x4), z_ok)


def test_stream_refuses_a_batch_past_the_table():
    from rave_amd import config as rcfg
    from rave_amd.streaming import StreamingRAVE
    cfg = rcfg.causal(capacity=8)
    m = _model(cfg, speaker_rows=2)
    s = StreamingRAVE(m, batch=3, block=2048, graph=False)
    x = torch.from_numpy(audio(3, 2048)).to(DEV)
    z0 = s.encode(x)                                        # shared mode: any batch
    m.set_speaker(embs(0, 1))
    with pytest.raises(ValueError):
        s.encode(x)
    m.set_speaker(emb(0))
    assert s.encode(x).shape == z0.shape


# ------------------------------------------------------------------ 9. shared mode
def test_shared_mode_above_the_table_size():
    """A model that only ever gets 1-D speakers is not bound by speaker_rows:
    B = 65 (above the 64 rows) runs and matches the oracle."""
    from oracle.rave_oracle import Oracle
    from rave_amd import config as rcfg
    cfg = rcfg.v2(capacity=8)
    p, spk = _params(cfg)
    m = _model(cfg)
    assert m.speaker_rows == 64
    B, T = 65, 1024
    x = audio(B, T)
    m.set_speaker(emb(3))
    y = m.forward(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert not m.per_row_speakers
    want = np.asarray(Oracle(cfg, p, emb(3), hk=m.hk).forward(x))
    err = maxabs(y, want)
    print(f"shared B=65: max-abs vs oracle {err:.3e}")
    assert err <= TOL
