"""Training losses on the HIP path.

CombinationEnhanceLoss is the reference's `--loss_func=CombinationEnhance` (loss/loss_base.py:28-29:
Combined_Loss(["mse", "charbonnier", "gaussian3D"], [1, 1, 1]); the terms are loss/loss_functions/
enhancement_losses.py:18-278), the loss of its two image-enhancement recipes (projects/run_cmr.sh, run_micro.sh),
as one fused forward + gradient op (csrc/loss.hip). There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, kernels

# Combined_Loss's GaussianDeriv3D_Loss(sigmas=[0.25, 0.5, 1.0], sigmas_T=[0.25, 0.5, 0.5]) (enhancement_losses.py:264)
SIGMAS = (0.25, 0.5, 1.0)       # along H and W
SIGMAS_T = (0.25, 0.5, 0.5)     # along T
HALFWIDTH = 3                   # in sigmas (enhancement_losses.py:190)
TAPS = 7                        # taps per factor in the kernel's table, centred at index 3


def _deriv_factor(sigma: float) -> np.ndarray:
    """The sampled first derivative of a Gaussian, normalised by its absolute sum (get_gaussionand_derivatives_1D /
    gaussian_fucntion, enhancement_losses.py:106-147; voxel size 1), float64. Python's round() is half-to-even, as
    in the reference: half-widths round(0.75) = 1, round(1.5) = 2, round(3.0) = 3."""
    hw = round(HALFWIDTH * sigma)
    x = np.arange(2 * hw + 1, dtype=np.float64) - hw
    d = 1.0 / np.sqrt(2 * np.pi * sigma * sigma) * (-x / (sigma * sigma)) * np.exp(-(x * x) / (2 * sigma * sigma))
    return d / np.sum(np.abs(d))


def enhance_factors():
    """Per stencil k the 1-D factors (fT, fH, fW), float64, whose outer product fT[t] fH[h] fW[w] is the reference's
    conv3d weight [0, 0, t, h, w]: create_window_3d builds window[x, y, z] = D_sigma[x] D_sigma[y] D_sigmaT[z], divides
    by sum|window| (1 up to rounding; folded into fT here), and GaussianDeriv3D_Loss permutes it to (z, x, y) =
    (T, H, W)."""
    out = []
    for s, st in zip(SIGMAS, SIGMAS_T):
        fh, fw, ft = _deriv_factor(s), _deriv_factor(s), _deriv_factor(st)
        total = np.sum(np.abs(fh)) * np.sum(np.abs(fw)) * np.sum(np.abs(ft))   # = sum |outer product|
        out.append((ft / total, fh, fw))
    return out


def enhance_taps_host() -> torch.Tensor:
    """The kernel's (3, 3, 7) f32 table: stencil k, axis (T, H, W), taps centred at index 3, zeros past the half-width."""
    tab = np.zeros((3, 3, TAPS), dtype=np.float64)
    for k, fs in enumerate(enhance_factors()):
        for a, f in enumerate(fs):
            hw = (len(f) - 1) // 2
            tab[k, a, TAPS // 2 - hw:TAPS // 2 + hw + 1] = f
    return torch.from_numpy(tab.astype(np.float32))


_taps_cache: dict = {}


def enhance_taps(device) -> torch.Tensor:
    """enhance_taps_host() on `device`, uploaded once per device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _taps_cache:
        with _lib.plain_tensors():   # a plain tensor even when first built in an EvalStep: training reuses it
            _taps_cache[device] = enhance_taps_host().to(device)
    return _taps_cache[device]


class CombinationEnhanceLoss:
    """loss(outputs, targets, weights=None) = mse + charbonnier(eps 1e-3) + gaussian3D of (B, 1, T, H, W) tensors,
    called like the reference's Combined_Loss. The scalar f32 loss back-propagates to `outputs`; the last call's
    (mse, charbonnier, gaussian3D) are kept in `.components`, a detached length-3 device tensor.

    Deviations from the reference, all deliberate:
      * NaN handling: the reference checks isnan on the host (three device syncs per step) and raises, or drops a NaN
        term from the sum. This op never syncs, so it can sit in a captured graph: a NaN in the inputs propagates to
        the loss.
      * arithmetic is f32 whatever the input dtypes; under autocast the reference's conv3d runs in bf16.
      * per-sample `weights` are not implemented (the reference trainer never passes them, trainer_base.py:168), nor
        is complex_i (get_loss_func never sets it).
    C != 1 raises: the reference's conv3d(groups=C) on its (1, 1, kT, kH, kW) weight only runs for C == 1. With T, H
    or W of 1 the gaussian term and its gradient are exactly 0 (every factor's centre tap is 0) and are skipped."""

    def __init__(self):
        self.taps_host = enhance_taps_host()
        self._taps = {}          # device -> the table there
        self.components = None

    def __call__(self, outputs, targets, weights=None):
        if weights is not None:
            raise NotImplementedError("CombinationEnhanceLoss: per-sample weights are not implemented")
        taps = self._taps.get(outputs.device)
        if taps is None:
            with _lib.plain_tensors():   # as in enhance_taps
                taps = self._taps[outputs.device] = self.taps_host.to(outputs.device)
        loss, self.components = kernels.enhance_loss(outputs, targets, taps)
        return loss
