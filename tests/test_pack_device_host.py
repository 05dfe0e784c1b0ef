"""rave_conv1d_pack_weight_device at the C boundary, host side (no GPU): the symbol, the ABI
version, and its refusals -- the host packer's, in the host packer's order, with the host
packer's status codes, made before anything touches the GPU."""
import ctypes as C

import pytest

NAME = "rave_conv1d_pack_weight_device"
BUF = (C.c_float * 4)()
P = C.cast(BUF, C.c_void_p)          # dummy non-null pointer: every call below is refused before it is read


def _N():
    from rave_amd import _native as N
    return N


def _both(w=P, c_in=16, c_out=16, kernel=3, stride=1, dilation=1, transposed=0, out_shift=0, packed=P):
    """(status, message) of the device packer and of the host packer for the same arguments."""
    N = _N()
    rc_d = N.lib.rave_conv1d_pack_weight_device(w, c_in, c_out, kernel, stride, dilation, transposed, out_shift,
                                                packed, None)
    msg_d = N.lib.rave_last_error().decode()
    rc_h = N.lib.rave_conv1d_pack_weight(w, c_in, c_out, kernel, stride, dilation, transposed, out_shift, packed)
    msg_h = N.lib.rave_last_error().decode()
    return rc_d, msg_d, rc_h, msg_h


def _refused(status, text, **kw):
    N = _N()
    rc_d, msg_d, rc_h, msg_h = _both(**kw)
    assert rc_h == getattr(N, status) and msg_h == "pack_weight: " + text, (rc_h, msg_h)
    assert rc_d == rc_h and msg_d == "pack_weight_device: " + text, (rc_d, msg_d)


def test_symbol_and_abi():
    N = _N()
    assert NAME in N.EXPORTS and hasattr(N.lib, NAME)
    assert N.ABI_VERSION == 21 and N.lib.rave_abi_version() == 21
    assert N.lib.rave_conv1d_pack_weight_device.argtypes[-2:] == [C.c_void_p, C.c_void_p]
    assert callable(N.pack_conv_weight_device)


def test_torch_ops_are_registered():
    import torch
    from rave_amd import cc  # noqa: F401  (loads the op library)
    assert torch.ops.rave_amd.pack_conv1d_device_ and torch.ops.rave_amd.pack_conv1d
    assert torch.ops.rave_amd.conv1d_packed_size(40, 24, 3, 1, 1, False) == 3 * 16 * 3 * 128
    assert torch.ops.rave_amd.conv1d_packed_size(40, 24, 5, 1, 1, False) == -1


@pytest.mark.parametrize("kw", [dict(w=None), dict(packed=None), dict(w=None, packed=None)])
def test_null_pointer(kw):
    _refused("RAVE_ERR_ARG", "null pointer", **kw)


@pytest.mark.parametrize("kw", [dict(c_in=0), dict(c_out=0), dict(kernel=0), dict(stride=0), dict(dilation=0),
                                dict(c_in=-3), dict(c_out=-1)])
def test_bad_shape(kw):
    _refused("RAVE_ERR_ARG", "bad shape", **kw)


@pytest.mark.parametrize("kw", [dict(kernel=5), dict(kernel=3, stride=2), dict(kernel=4, stride=1),
                                dict(kernel=8, stride=2), dict(transposed=1, kernel=4, stride=4),
                                dict(transposed=1, kernel=3, stride=2)])
def test_unsupported_layer_shape(kw):
    _refused("RAVE_ERR_UNSUPPORTED", "unsupported layer shape", **kw)


@pytest.mark.parametrize("r,shift", [(2, 2), (4, 1), (4, 3), (4, -1), (2, 5)])
def test_transposed_out_shift(r, shift):
    _refused("RAVE_ERR_ARG", "transposed out_shift must be 0 or stride/2", transposed=1, kernel=2 * r, stride=r,
             out_shift=shift)


def test_refusals_come_in_the_host_packers_order():
    """Arguments that break two or more rules at once get the earlier rule's refusal."""
    # null pointer before bad shape, unsupported shape and out_shift
    _refused("RAVE_ERR_ARG", "null pointer", w=None, c_in=0)
    _refused("RAVE_ERR_ARG", "null pointer", packed=None, kernel=5)
    _refused("RAVE_ERR_ARG", "null pointer", w=None, transposed=1, kernel=4, stride=2, out_shift=2)
    # bad shape before unsupported shape and out_shift
    _refused("RAVE_ERR_ARG", "bad shape", c_out=0, kernel=5)
    _refused("RAVE_ERR_ARG", "bad shape", dilation=0, kernel=3, stride=2)
    _refused("RAVE_ERR_ARG", "bad shape", c_in=0, transposed=1, kernel=4, stride=2, out_shift=2)
    # unsupported shape before out_shift
    _refused("RAVE_ERR_UNSUPPORTED", "unsupported layer shape", transposed=1, kernel=6, stride=2, out_shift=2)
    # all four at once
    _refused("RAVE_ERR_ARG", "null pointer", w=None, c_in=0, transposed=1, kernel=6, stride=2, out_shift=2)


def test_module_cache_key_is_not_an_address():
    """The image's cache key names the weight tensor itself (a weak reference) beside its
    [data_ptr, _version]; a module that has packed nothing matches no tensor."""
    from rave_amd import cc
    conv = cc.Conv1d(40, 24, 3, padding=(1, 1))
    assert conv.packed_for is None and conv.packed.numel() == 0
    assert conv.packed_size == 3 * 16 * 3 * 128
    up = cc.ConvTranspose1d(32, 16, 4, stride=2, padding=1)
    assert up.packed_size == 32 * 2 * 128
