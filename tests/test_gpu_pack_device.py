"""The device-side weight packer (rave_conv1d_pack_weight_device, rave_amd::pack_conv1d_device_)
and cc._PackedConv over it.

Image: the reference is the host packer into zeros; the device image goes into a destination
pre-filled with NaN (with NaN guard floats behind it) and must equal it bit for bit, compared as
uint32, over the whole rave_conv1d_packed_size.  It is a copy: there is no tolerance.

Module: after any weight change the output is the output of a freshly constructed module holding
the same weights, bit for bit; `packed` keeps one storage; nothing on the path syncs the host."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16
CIT = {1: 32, 3: 16, 7: 8, 4: 16, 8: 8}                # input channels per K chunk, per family
C_OUT = (1, 16, 127, 128, 129, 300)
T_C_IN = (1, 31, 32, 33, 72)
T_C_OUT = (1, 3, 16, 31, 33, 136)


def _N():
    from rave_amd import _native as N
    return N


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _c_ins(k):
    return (1, CIT[k] - 1, CIT[k], CIT[k] + 1, 40, 136)


def _weight(shape, seed):
    """Distinct, sign-mixed values with a few exact zeros, negative zeros and a denormal: a
    permutation copy must carry every bit pattern."""
    w = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    flat = w.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = 1e-42
    return w


def _device_image(w, c_in, c_out, k, s, d, transposed, shift, calls=1):
    """The device packer's image of `w` (numpy) as uint32, from a NaN-filled destination."""
    N = _N()
    n = int(N.lib.rave_conv1d_packed_size(c_in, c_out, k, s, d, int(transposed)))
    wd = torch.from_numpy(w).to(DEV)
    outs = []
    for _ in range(calls):
        dst = torch.full((n + GUARD,), float("nan"), device=DEV)
        N.pack_conv_weight_device(wd.data_ptr(), c_in, c_out, k, s, d, transposed, shift, dst.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dst[n:]).all()), "wrote past packed_size"
        outs.append(dst[:n].cpu().numpy().view(np.uint32))
    return outs if calls > 1 else outs[0]


def _check(c_in, c_out, k, s, d, transposed, shift, seed=0):
    N = _N()
    shape = (c_in, c_out, k) if transposed else (c_out, c_in, k)
    w = _weight(shape, seed)
    ref = N.pack_conv_weight(w, c_in, c_out, k, s, d, transposed, shift).view(np.uint32)
    got = _device_image(w, c_in, c_out, k, s, d, transposed, shift)
    assert got.shape == ref.shape
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (c_in, c_out, k, s, d, transposed, shift, bad[:8], got[bad[:8]], ref[bad[:8]])


# ================================================================== 1. the image
@pytest.mark.parametrize("k,s", [(1, 1), (3, 1), (7, 1), (4, 2), (8, 4)])
def test_conv_image_is_the_host_packers(k, s):
    for c_in in _c_ins(k):
        for c_out in C_OUT:
            _check(c_in, c_out, k, s, 1, False, 0, seed=c_in * 1000 + c_out)


def test_dilation_does_not_change_the_image():
    _check(40, 129, 3, 1, 9, False, 0)
    w = _weight((129, 40, 3), 1)
    assert np.array_equal(_device_image(w, 40, 129, 3, 1, 9, False, 0), _device_image(w, 40, 129, 3, 1, 1, False, 0))


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("half", [False, True])
def test_transposed_image_is_the_host_packers(r, half):
    """out_shift 0: one row group, and a tail up to the larger layout's size.  out_shift r/2: two
    groups, group 0's c_out * r/2 rows padded to a multiple of 64 (these c_out give counts on and
    off a multiple: r = 4 with c_out 16 is 32 -> 64 rows, c_out 136 is 272 -> 320)."""
    shift = r // 2 if half else 0
    for c_in in T_C_IN:
        for c_out in T_C_OUT:
            _check(c_in, c_out, 2 * r, r, 1, True, shift, seed=c_in * 1000 + c_out)


def test_transposed_group0_rows_at_a_multiple_of_64():
    _check(33, 32, 4, 2, 1, True, 1)       # c_out * q0 = 32 -> 64 rows
    _check(33, 64, 4, 2, 1, True, 1)       # 64: no padding rows
    _check(33, 32, 8, 4, 1, True, 2)       # 64
    _check(33, 48, 8, 4, 1, True, 2)       # 96 -> 128


def test_production_upsampler_and_two_calls():
    """The v2 decoder's widest image, ConvTranspose1d(1024, 512, 4, stride 2): over 2 M floats."""
    N = _N()
    w = _weight((1024, 512, 4), 5)
    ref = N.pack_conv_weight(w, 1024, 512, 4, 2, 1, True, 1).view(np.uint32)
    a, b = _device_image(w, 1024, 512, 4, 2, 1, True, 1, calls=2)
    assert ref.size > 2_000_000 and np.array_equal(a, ref) and np.array_equal(a, b)
    w = _weight((300, 136, 7), 6)
    a, b = _device_image(w, 136, 300, 7, 1, 1, False, 0, calls=2)
    assert np.array_equal(a, b)


def test_torch_op_packs_in_place_and_checks_its_tensors():
    from rave_amd import cc  # noqa: F401
    N = _N()
    op = torch.ops.rave_amd.pack_conv1d_device_
    w = torch.from_numpy(_weight((24, 40, 3), 2)).to(DEV).requires_grad_(True)
    n = int(torch.ops.rave_amd.conv1d_packed_size(40, 24, 3, 1, 1, False))
    dst = torch.full((n,), float("nan"), device=DEV)
    out = op(w.detach(), dst, 40, 24, 3, 1, 1, False, 0)
    assert out.data_ptr() == dst.data_ptr() and out.grad_fn is None
    ref = N.pack_conv_weight(w.detach().cpu().numpy(), 40, 24, 3, 1, 1, False, 0)
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    host = torch.ops.rave_amd.pack_conv1d(w, 40, 24, 3, 1, 1, False, 0, 0)       # registered and unchanged
    assert host.device.type == "cpu" and np.array_equal(host.numpy().view(np.uint32), ref.view(np.uint32))
    wd = w.detach()
    with pytest.raises(ValueError):
        op(wd.cpu(), dst, 40, 24, 3, 1, 1, False, 0)
    with pytest.raises(ValueError):
        op(wd, dst.cpu(), 40, 24, 3, 1, 1, False, 0)
    with pytest.raises(ValueError):
        op(wd.double(), dst, 40, 24, 3, 1, 1, False, 0)
    with pytest.raises(ValueError):
        op(wd.transpose(0, 1), dst, 40, 24, 3, 1, 1, False, 0)
    with pytest.raises(ValueError):
        op(wd, dst[:-1], 40, 24, 3, 1, 1, False, 0)
    with pytest.raises(ValueError):
        op(wd[:-1], dst, 40, 24, 3, 1, 1, False, 0)
    with pytest.raises(NotImplementedError):
        op(torch.zeros(24, 40, 5, device=DEV), dst, 40, 24, 5, 1, 1, False, 0)


# ================================================================== 2. the modules
def _conv():
    from rave_amd import cc
    return cc.Conv1d(40, 24, 3, padding=(1, 1)).to(DEV)


def _convt():
    from rave_amd import cc
    cc.use_transposed_grad(True)
    try:
        return cc.ConvTranspose1d(32, 16, 4, stride=2, padding=1, bias=True).to(DEV)
    finally:
        cc.use_transposed_grad(False)


def _fresh_output(make, weight, bias, x):
    """The output of a newly constructed module holding these weights."""
    m = make()
    with torch.no_grad():
        m.weight.copy_(weight)
        if bias is not None:
            m.bias.copy_(bias)
        return m(x)


def _same(a, b):
    return bool((a.detach().view(torch.int32) == b.detach().view(torch.int32)).all())


@pytest.mark.parametrize("make", [_conv, _convt], ids=["conv", "convt"])
def test_module_follows_its_weight(make):
    torch.manual_seed(0)
    m = make()
    x = torch.randn(2, m.c_in, 50, device=DEV)
    y = m(x)
    assert y.grad_fn is not None and _same(y, _fresh_output(make, m.weight, m.bias, x))
    storage = m.packed.untyped_storage().data_ptr()
    assert m.packed.is_cuda and m.packed.numel() == m.packed_size

    before = y.detach().clone()
    m.weight.data.add_(0.01 * torch.randn_like(m.weight))          # moves neither the address nor _version
    y = m(x)
    assert not _same(y, before) and _same(y, _fresh_output(make, m.weight, m.bias, x))

    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for _ in range(2):
        before = y.detach().clone()
        opt.zero_grad()
        m(x).square().mean().backward()
        opt.step()
        y = m(x)
        assert not _same(y, before) and _same(y, _fresh_output(make, m.weight, m.bias, x))
        assert m.packed.untyped_storage().data_ptr() == storage   # one buffer across steps
    m.prepare()
    assert m.packed.untyped_storage().data_ptr() == storage and _same(m(x), y)


@pytest.mark.parametrize("make", [_conv, _convt], ids=["conv", "convt"])
def test_module_under_weight_norm(make):
    torch.manual_seed(1)
    m = torch.nn.utils.weight_norm(make())
    x = torch.randn(2, m.c_in, 50, device=DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    storage = None
    for step in range(3):
        y = m(x)
        w = torch._weight_norm(m.weight_v, m.weight_g, 0)
        assert _same(y, _fresh_output(make, w, m.bias, x)), step
        if storage is None:
            storage = m.packed.untyped_storage().data_ptr()
        assert m.packed.untyped_storage().data_ptr() == storage
        opt.zero_grad()
        y.square().mean().backward()
        assert m.weight_g.grad is not None and m.weight_v.grad is not None
        opt.step()


@pytest.mark.parametrize("make", [_conv, _convt], ids=["conv", "convt"])
def test_recycled_address_gets_the_new_weights_output(make):
    """Forward, drop the weight, install a new parameter of the same shape: the caching allocator
    normally hands out the same address (recorded, not required).  The output is the new weight's."""
    torch.manual_seed(2)
    m = make()
    x = torch.randn(2, m.c_in, 50, device=DEV)
    with torch.no_grad():
        old = m(x).clone()
        old_ptr, values = m.weight.data_ptr(), torch.randn(m.weight.shape) * 0.1
        del m.weight
        torch.cuda.synchronize()
        new = torch.nn.Parameter(values.to(DEV))       # one allocation of the freed block's size, version 0
        m.weight = new
        recycled = new.data_ptr() == old_ptr
        print(f"recycled address: {recycled} (version {new._version})")
        y = m(x)
    assert not _same(y, old) and _same(y, _fresh_output(make, new, m.bias, x))


def test_host_path_key_is_the_tensor_not_its_address():
    """split16 keeps the host packer and its cache; the key names the tensor object."""
    from rave_amd import cc
    cc.set_precision("split16")
    try:
        m = cc.Conv1d(32, 32, 3, padding=(1, 1)).to(DEV)
    finally:
        cc.set_precision("f32")
    x = torch.randn(1, 32, 64, device=DEV)
    with torch.no_grad():
        y0 = m(x)
        assert m.packed_for() is m.weight and m.packed_key == [m.weight.data_ptr(), m.weight._version]
        image = m.packed
        assert m(x) is not None and m.packed is image                 # cached: no repack
        ptr, values = m.weight.data_ptr(), torch.randn(m.weight.shape) * 0.1
        del m.weight
        m.weight = torch.nn.Parameter(values.to(DEV))
        print(f"recycled address: {m.weight.data_ptr() == ptr}")
        y1 = m(x)
    assert m.packed is not image and not _same(y0, y1) and m.packed_for() is m.weight


# ================================================================== 3. no host sync
def test_forward_after_a_weight_change_does_not_sync():
    m = _conv()
    x = torch.randn(2, 40, 50, device=DEV)
    m(x)                                                               # the buffer exists
    w = m.weight.detach()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ops.rave_amd.pack_conv1d(w, 40, 24, 3, 1, 1, False, 0, 0)   # control: copies the weight to the host
            control = False
        except RuntimeError:
            control = True
        if control:
            with torch.no_grad():
                m.weight.add_(0.01)
            y = m(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not control:
        pytest.skip("this torch build does not raise on a synchronising copy under set_sync_debug_mode('error')")
    assert _same(y, _fresh_output(_conv, m.weight, m.bias, x))


# ================================================================== 4. end to end
def _generator():
    from rave_amd import cc, modules as M
    cc.use_transposed_grad(True)
    try:
        return M.GeneratorV2(data_size=16, capacity=16, ratios=(2, 4), latent_size=16, kernel_size=3, dilations=[1, 3],
                             activation="leaky", adain=False, noise=None).to(DEV)
    finally:
        cc.use_transposed_grad(False)


def _host_prepare(gen):
    """prepare() through the host op, as before the device packer, marked current."""
    from rave_amd import cc
    for m in gen.modules():
        if isinstance(m, cc._PackedConv):
            w = m.weight
            m.packed = torch.ops.rave_amd.pack_conv1d(w, m.c_in, m.c_out, m.kernel, m.stride, m.dilation, m.transposed,
                                                      m.out_shift, m.precision).to(w.device)


def _train(gen, z, host):
    from rave_amd import cc
    convs = [m for m in gen.modules() if isinstance(m, cc._PackedConv)]
    if host:           # the forward reads whatever `packed` holds
        for m in convs:
            m._packed_weight = (lambda mod: lambda x: mod.packed)(m)
    opt = torch.optim.SGD(gen.parameters(), lr=0.05)
    for _ in range(3):
        if host:
            _host_prepare(gen)
        opt.zero_grad()
        gen(z).square().mean().backward()
        opt.step()
    return [p.detach().clone() for p in gen.parameters()]


def test_three_sgd_steps_match_the_host_packed_tree():
    torch.manual_seed(3)
    a = _generator()
    torch.manual_seed(3)
    b = _generator()
    assert all(_same(p, q) for p, q in zip(a.parameters(), b.parameters()))
    z = torch.randn(2, 16, 33, device=DEV)
    start = [p.detach().clone() for p in a.parameters()]
    pa, pb = _train(a, z, host=False), _train(b, z, host=True)
    assert len(pa) == len(pb) and len(pa) > 10
    assert any(not _same(p, s) for p, s in zip(pa, start))             # the steps moved the weights
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert _same(p, q), i
    # the head's tree packed on the device, into buffers of its own
    from rave_amd import cc
    for m in a.modules():
        if isinstance(m, cc._PackedConv):
            assert m.packed.is_cuda and m.packed.numel() == m.packed_size

