#!/usr/bin/env python3
"""Check the pitch tests' CPU reference (tests/pitch_ref.py) against the
reference's own ``rave/pitch_utils.py``: ``estimate`` / ``_frame`` / ``_diff`` /
``_search`` (:15-86), ``get_pitch`` (:90-96), ``one_hot`` (:98-104) and the
'abs' arithmetic of ``quantize_f0_norm`` / ``get_f0_norm`` (:112-127).

Needs a checkout of the reference (make_golden.py's loader path-imports it).
``pitch_utils`` imports ``torchfcpe`` and loads the FCPE model onto ``cuda:2``
at module level; refshim/torchfcpe.py stands in for the package, and librosa is
one of the loader's empty stand-ins.  ``get_f0_norm`` itself takes its contour
from FCPE, so its quantiser is checked by handing the module a stand-in
``extract_utterance_fcpe`` that returns the YIN contour instead.

For every case of tests/pitch_ref.py, in float64 and float32: the sliced cmdf
(1e-12 / 1e-5 relative to its largest value; float32 differs only by the
thread-dependent order of the FFT), the period index and f0; the same in
float64 for every case of the edge sweep (SWEEP); for the table of
tests/pitch_ref.py and each case's contour: the one-hot and the normalised
log-f0.  Writes nothing; runs on the CPU only.

Usage:  python tests/golden/make_pitch_check.py
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
from tests import pitch_ref as R  # noqa: E402  (make_golden put the repository root on sys.path)


def main():
    G.install_shims()
    P = importlib.import_module("rave.pitch_utils")
    for case, c in R.CASES.items():
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
            x = torch.tensor(R.inputs(case), dtype=dtype)
            tau_min, tau_max, L, stride, frames = R.geometry(case)
            fr = P._frame(x, L, stride)
            assert torch.equal(fr, R.frame(x, L, stride)) and fr.shape[-2] == frames
            cmdf = P._diff(fr, tau_max)[..., tau_min:]
            mine, idx, f0 = R.analyse(x, c["sr"], c["pmin"], c["pmax"], R.frame_stride(case))
            dev = float((cmdf - mine).abs().max() / mine.abs().max())
            assert dev <= tol, (case, dtype, dev)
            assert torch.equal(P._search(mine, tau_max, R.THRESHOLD), idx)
            if "block" in c:
                ref_f0 = P.get_pitch(x, c["block"], c["sr"], c["pmin"], c["pmax"])
            else:
                ref_f0 = P.estimate(x, c["sr"], c["pmin"], c["pmax"], c["stride"], R.THRESHOLD)
            same = torch.equal(ref_f0, f0)
            print(f"  {case} {str(dtype)[6:]}: cmdf off by {dev:.1e}, f0 {'equal' if same else 'DIFFERS'} "
                  f"({int((f0 > 0).sum())} of {f0.numel()} voiced)")
            assert same or dtype == torch.float32, case
    # the edge sweep's inputs (tests/pitch_ref.py SWEEP), in float64: frames, cmdf
    # (NaN where the reference's is: the rows holding a NaN or inf), index and f0
    worst = 0.0
    for name, c in R.SWEEP.items():
        x = torch.tensor(R.sweep_input(name), dtype=torch.float64)
        fr = P._frame(x, c["L"], c["stride"])
        assert torch.equal(torch.nan_to_num(fr), torch.nan_to_num(R.frame(x, c["L"], c["stride"]))), name
        assert fr.shape[-2] == c["frames"], name
        cmdf = P._diff(fr, c["tau_max"])[..., c["tau_min"]:]
        mine, idx, f0 = R.analyse(x, c["sr"], c["pmin"], c["pmax"], c["stride_s"], c["threshold"])
        assert torch.equal(torch.isnan(cmdf), torch.isnan(mine)), name
        a, b = torch.nan_to_num(cmdf), torch.nan_to_num(mine)
        dev = float((a - b).abs().max() / b.abs().max().clamp(min=1.0))
        worst = max(worst, dev)
        assert dev <= 1e-12, (name, dev)
        assert torch.equal(P._search(mine, c["tau_max"], c["threshold"]), idx), name
        ref_f0 = P.estimate(x, c["sr"], c["pmin"], c["pmax"], c["stride_s"], c["threshold"])
        assert torch.equal(ref_f0, f0), name
        t = R.sweep_truth(name)
        assert torch.equal(idx, torch.from_numpy(t["idx_fft64"])) and bool((idx.numpy()[t["poisoned"]] == 0).all()), name
    print(f"  sweep: {len(R.SWEEP)} cases in float64, cmdf off by at most {worst:.1e}, index and f0 equal")
    # the quantiser, fed the YIN contour in FCPE's place: (B, frames, 1), 0 = unvoiced
    contours = [torch.from_numpy(R.table_f0()).reshape(1, -1)]
    contours += [R.reference(case, "float32")[2].reshape(-1, R.geometry(case)[4]) for case in R.CASES]
    for f0 in contours:
        for dtype in (torch.float64, torch.float32):
            f = f0.to(dtype)
            P.extract_utterance_fcpe = lambda y, sr, n, f=f: f.clone()[..., None]
            hot, norm = P.get_f0_norm(f, None, None, 44100, 1024)
            assert torch.equal(hot, R.f0_one_hot(f).to(hot.dtype)), "one-hot"
            assert torch.equal(hot.argmax(-1), R.f0_classes(f))
            mine = R.f0_norm(f)
            assert torch.equal(torch.isnan(norm), torch.isnan(mine))
            assert torch.equal(torch.nan_to_num(norm), torch.nan_to_num(mine)), "normalised log-f0"
    print("tests/pitch_ref.py matches the reference's pitch_utils")


if __name__ == "__main__":
    main()
