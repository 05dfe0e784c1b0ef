#!/usr/bin/env python3
"""Check the spectral-loss tests' CPU reference (tests/stft_loss_ref.py) against
the reference's own ``rave/stft_loss.py``: ``stft`` (:12-35),
``SpectralConvergenceLoss`` (:38-55), ``LogSTFTMagnitudeLoss`` (:58-75) and the
averaging of ``MultiResolutionSTFTLoss.forward`` (:125-144), with the
resolutions of ``rave/model.py:191-196``.

Needs a checkout of the reference (make_golden.py's loader path-imports it).
``STFTLoss.__init__`` puts its window on ``cuda:2``, so the losses are composed
here from the module's functions, as ``STFTLoss.forward`` and
``MultiResolutionSTFTLoss.forward`` compose them.

For every input of tests/stft_loss_ref.py, in float64: the magnitudes, the two
terms of every resolution and the two means, 1e-12 relative; the gradient of
both means with respect to the predicted signal, 1e-12 relative L2.  Writes
nothing; runs on the CPU only.

Usage:  python tests/golden/make_stft_loss_check.py
"""
from __future__ import annotations

import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
from tests import stft_loss_ref as R  # noqa: E402  (make_golden put the repository root on sys.path)

TOL = 1e-12


def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).norm() / b.norm())


def main():
    G.install_shims()
    S = importlib.import_module("rave.stft_loss")
    sc_fn, mag_fn = S.SpectralConvergenceLoss(), S.LogSTFTMagnitudeLoss()
    assert R.fork_resolutions(44100) == ((2048, 220, 1102), (4096, 441, 2205), (512, 88, 441))
    cases = [(f"multires {c}", R.mr_inputs(c), R.fork_resolutions()) for c in R.MR_CASES]
    cases.append(("odd geometry", R.odd_inputs(), R.ODD))
    for name, (pred, target), res in cases:
        t = torch.from_numpy(target).double()

        def theirs(p):
            sc = mag = 0.0
            terms = []
            for fs, ss, wl in res:
                window = torch.hann_window(wl, dtype=torch.float64)
                x_mag, y_mag = S.stft(p, fs, ss, wl, window), S.stft(t, fs, ss, wl, window)
                terms.append((sc_fn(x_mag, y_mag), mag_fn(x_mag, y_mag)))
                sc, mag = sc + terms[-1][0], mag + terms[-1][1]
            return sc / len(res), mag / len(res), terms

        p = torch.from_numpy(pred).double().requires_grad_(True)
        sc, mag, terms = theirs(p)
        g_sc, g_mag = (torch.autograd.grad(v, p, retain_graph=True)[0] for v in (sc, mag))
        q = torch.from_numpy(pred).double().requires_grad_(True)
        msc, mmag = R.mr_loss(q, t, res)
        mine = R.mr_terms(q, t, res)
        h_sc, h_mag = (torch.autograd.grad(v, q, retain_graph=True)[0] for v in (msc, mmag))
        worst = max(rel(msc, sc), rel(mmag, mag), rel(h_sc, g_sc), rel(h_mag, g_mag))
        for (a, b), (c, d) in zip(mine, terms):
            worst = max(worst, rel(a, c), rel(b, d))
        for fs, ss, wl in res:
            theirs_mag = S.stft(t, fs, ss, wl, torch.hann_window(wl, dtype=torch.float64))
            mine_mag = R.mr_mag(t, fs, ss, wl)
            assert theirs_mag.shape == mine_mag.shape == (t.shape[0], 1 + t.shape[1] // ss, fs // 2 + 1)
            worst = max(worst, rel(mine_mag, theirs_mag))
        print(f"  {name}: sc {float(sc):.12g} mag {float(mag):.12g}, off by {worst:.1e}; "
              f"{R.clamped_share(q.detach(), res):.1e} of pred's bins under the clamp")
        assert worst <= TOL, (name, worst)
    print("tests/stft_loss_ref.py matches the reference's stft_loss")


if __name__ == "__main__":
    main()
