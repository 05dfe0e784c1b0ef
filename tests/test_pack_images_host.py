"""The host packers' images, byte for byte (no GPU): every weight and filter packer of the
library against sha256 digests recorded from the commit before the packers were folded onto
one core (csrc/pack_shared.h), and every *_packed_size against the size recorded there.

Every weight carries, as GEMM rows: an all-zero row; a row whose largest magnitude is exactly
a power of two and one a single ulp below it (both edges of the row exponent); a value whose
bf16 rounding carries into the exponent; and a value that falls below f16's subnormal range
once the row is scaled.

Recording (against the library the digests are to come from, here a build of the parent):
    RAVE_AMD_LIB_VARIANT=parent python -m tests.test_pack_images_host
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_images.json")

# (name, kernel, stride, dilation, transposed, out_shift)
LAYERS = ([("k1", 1, 1, 1, 0, 0), ("k3d1", 3, 1, 1, 0, 0), ("k3d3", 3, 1, 3, 0, 0), ("k3d9", 3, 1, 9, 0, 0),
           ("k7", 7, 1, 1, 0, 0), ("k4s2", 4, 2, 1, 0, 0), ("k8s4", 8, 4, 1, 0, 0)] +
          [(f"t{r}o{o}", 2 * r, r, 1, 1, o) for r in (2, 4) for o in (0, r // 2)])
PAIRS = [(16, 16), (40, 24), (136, 16)]
UNIT_C = [64, 128, 256, 512]
MODES = ["split16", "ring", "bf3", "f32"]          # f32: the plain fp32 packers


def _N():
    from rave_amd import _native as N
    return N


def _prec(N, mode):
    return {"split16": N.PREC_SPLIT16, "ring": N.PREC_F32_RING, "bf3": N.PREC_BF16X3, "f32": N.PREC_F32}[mode]


def gemm_rows(rows, k, seed, top=0.25):
    """(rows, k) float32 weights, |w| <= 0.2 but for the crafted entries (rows >= 4, k >= 4)."""
    g = np.clip(0.1 * np.random.default_rng(seed).standard_normal((rows, k)), -0.2, 0.2).astype(np.float32)
    g[0] = 0.0                                                        # all-zero row
    g[1, 0] = -np.float32(top)                                        # max |w| exactly 2^-2
    g[2, 0] = np.nextafter(np.float32(0.25), np.float32(0))           # one ulp below it
    g[3, 1] = np.uint32(0x3F7FFFFF).view(np.float32)                  # bf16(0.99999994) == 1.0: carries
    g[3, 2] = np.float32(1e-12)                                       # row scale <= 16: far below 2^-24
    return g


def conv_weight(c_in, c_out, kernel, stride, transposed, seed):
    """Torch-layout weight whose GEMM rows are gemm_rows: (c_out, c_in, k), or for a transposed
    conv (c_in, c_out, 2 r), where row (co, phase) holds taps {p, p + r} of every input channel."""
    if not transposed:
        return gemm_rows(c_out, c_in * kernel, seed).reshape(c_out, c_in, kernel)
    g = gemm_rows(c_out * stride, c_in * 2, seed).reshape(c_out, stride, c_in, 2)
    return np.ascontiguousarray(g.transpose(2, 0, 3, 1)).reshape(c_in, c_out, 2 * stride)


def _entry(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "floats": int(a.size)}


def conv_images(mode):
    N = _N()
    out = {}
    for li, (name, k, s, d, tr, osh) in enumerate(LAYERS):
        for pi, (ci, co) in enumerate(PAIRS):
            w = conv_weight(ci, co, k, s, tr, seed=100 * li + pi)
            out[f"conv/{mode}/{name}/{ci}x{co}"] = _entry(
                N.pack_conv_weight(w, ci, co, k, s, d, bool(tr), osh, precision=_prec(N, mode)))
    return out


def unit_images(mode):
    N = _N()
    out = {}
    for C in UNIT_C:
        w1 = gemm_rows(C, 3 * C, seed=7000 + C).reshape(C, C, 3)
        w2 = gemm_rows(C, C, seed=8000 + C).reshape(C, C, 1)
        out[f"unit/{mode}/{C}"] = _entry(N.pack_unit_weight(w1, w2, C, precision=_prec(N, mode)))
    return out


def filter_images():
    """Head (16, 513) and tail (16, 16, 33) filters; one exponent per image, so both of its
    edges take an image each: largest magnitude 2^-2 ("pow2") and one ulp below ("ulp")."""
    N = _N()
    out = {}
    for edge, top in (("pow2", 0.25), ("ulp", np.nextafter(np.float32(0.25), np.float32(0)))):
        head = gemm_rows(16, 513, seed=9001, top=top)
        tail = gemm_rows(16, 16 * 33, seed=9002, top=top).reshape(16, 16, 33)
        for f32 in (False, True):
            m = "f32" if f32 else "split16"
            out[f"filter/head/{m}/{edge}"] = _entry(N.pack_edge_filter(head, True, 6, f32))
            out[f"filter/tail/{m}/{edge}"] = _entry(N.pack_edge_filter(tail, False, f32=f32))
    return out


def packed_sizes():
    lib = _N().lib
    out = {}
    for name, k, s, d, tr, _ in LAYERS:
        for ci, co in PAIRS:
            for fn in ("rave_conv1d_packed_size", "rave_conv1d_split_packed_size", "rave_conv1d_bf3_packed_size"):
                out[f"{fn}/{name}/{ci}x{co}"] = int(getattr(lib, fn)(ci, co, k, s, d, tr))
    for fn in ("rave_conv1d_packed_size", "rave_conv1d_split_packed_size", "rave_conv1d_bf3_packed_size"):
        out[f"{fn}/k5"] = int(getattr(lib, fn)(16, 16, 5, 1, 1, 0))                  # refused: -1
    for C in UNIT_C + [96]:                                                           # 96: refused
        for fn in ("rave_unit_packed_size", "rave_unit_split_packed_size", "rave_unit_bf3_packed_size"):
            out[f"{fn}/{C}"] = int(getattr(lib, fn)(C))
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _check(got, section="images"):
    want = {k: v for k, v in golden()[section].items() if k in got}
    assert sorted(want) == sorted(got)
    wrong = [k for k in got if got[k] != want[k]]
    assert not wrong, wrong


@pytest.mark.parametrize("mode", MODES)
def test_conv_images(mode):
    got = conv_images(mode)
    assert len(got) == len(LAYERS) * len(PAIRS)
    _check(got)


@pytest.mark.parametrize("mode", MODES)
def test_unit_images(mode):
    got = unit_images(mode)
    assert len(got) == len(UNIT_C)
    _check(got)


def test_filter_images():
    got = filter_images()
    assert len(got) == 8
    _check(got)


def test_packed_sizes():
    got = packed_sizes()
    _check(got, "sizes")
    # and every image above has the length its size entry point reports
    sizes, images = golden()["sizes"], golden()["images"]
    fn = {"split16": "rave_conv1d_split_packed_size", "ring": "rave_conv1d_split_packed_size",
          "bf3": "rave_conv1d_bf3_packed_size", "f32": "rave_conv1d_packed_size"}
    for key, e in images.items():
        kind, mode, *rest = key.split("/")
        if kind == "conv":
            assert e["floats"] == sizes[f"{fn[mode]}/{rest[0]}/{rest[1]}"], key
        elif kind == "unit":
            assert e["floats"] == sizes[f"{fn[mode].replace('conv1d', 'unit')}/{rest[0]}"], key


def test_golden_holds_exactly_these_cases():
    n_images = (len(MODES) * (len(LAYERS) * len(PAIRS) + len(UNIT_C))) + 8
    assert len(golden()["images"]) == n_images
    assert len(golden()["sizes"]) == 3 * (len(LAYERS) * len(PAIRS) + 1 + len(UNIT_C) + 1)


if __name__ == "__main__":
    images = filter_images()
    for m in MODES:
        images.update(conv_images(m))
        images.update(unit_images(m))
    with open(GOLDEN, "w") as f:
        json.dump({"images": images, "sizes": packed_sizes()}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(images)} images")
