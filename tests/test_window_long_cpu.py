"""No GPU: the large-window attention path (csrc/window_long.hip) at the host side -- the ABI declarations, the
constructor limits of WindowAttention, and the arithmetic relative-position index the kernels evaluate."""
import math
import os

import numpy as np
import pytest

from oracle import window as ow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry point -> number of arguments kernels.py passes
ARITY = {"lci_window_long_fwd": 9, "lci_window_long_bwd": 16, "lci_window_long_pad_ws_elems": 2,
         "lci_window_long_ws_bytes": 2, "lci_window_long_ws_items": 2, "lci_window_long_index": 4}


def test_header_declares_the_long_window_entry_points():
    from long_context_biomedical_imaging_amd import _lib
    abi, sigs = _lib.header()
    assert abi >= 43
    for name, n in ARITY.items():
        assert name in sigs, f"include/lci.h does not declare {name}"
        assert len(sigs[name][1]) == n, f"{name}: {len(sigs[name][1])} arguments declared, the binding passes {n}"
    lib = _lib.load()
    for name in ARITY:
        assert hasattr(lib, name), f"liblci.so does not export {name}"


def test_limits_are_exported():
    from long_context_biomedical_imaging_amd import kernels
    assert (kernels.WIN_MAX_TOKENS, kernels.WIN_LONG_MAX_TOKENS, kernels.WIN_LONG_MAX_TABLE) == (768, 4096, 29791)


@pytest.mark.parametrize("ws", [(32, 32, 8), (65, 65)])
def test_constructor_rejects_windows_beyond_the_limits(ws):
    from long_context_biomedical_imaging_amd import backbone_swin
    with pytest.raises(ValueError, match="window_size"):
        backbone_swin.WindowAttention(False, False, 32, 1, ws, qkv_bias=True)


@pytest.mark.parametrize("ws", [(32, 32), (16, 16, 16)])
def test_constructor_builds_large_windows(ws):
    from long_context_biomedical_imaging_amd import backbone_swin
    m = backbone_swin.WindowAttention(False, False, 32, 1, ws, qkv_bias=True)
    n = math.prod(ws)
    assert m.relative_position_bias_table.shape == (math.prod(2 * w - 1 for w in ws), 1)
    assert m.relative_position_index.shape == (n, n)


def test_prepartitioned_call_names_the_grid_path():
    import torch
    from long_context_biomedical_imaging_amd import _lib, kernels
    qkv = torch.zeros(1, 784, 96, dtype=torch.bfloat16)
    with pytest.raises(_lib.LciError, match="grid path"):
        kernels.window_attention(qkv, torch.zeros(1, 784, 784), None, 1, 1.0)


def rel_index(full, n):
    """The kernels' rel(q, k) restated: code(j) = sum_s coord_s(j) * W_s over the raster of the FULL window, W_s =
    prod_{t>s} (2 full_t - 1); rel = code(q) - code(k) + sum_s (full_s - 1) W_s."""
    wgt, t = [], 1
    for w in reversed(full):
        wgt.append(t)
        t *= 2 * w - 1
    wgt = wgt[::-1]
    coords = np.stack(np.unravel_index(np.arange(n), full), axis=1)          # raster position j of the full window
    code = (coords * np.array(wgt)).sum(1)
    c0 = sum((w - 1) * g for w, g in zip(full, wgt))
    return code[:, None] - code[None, :] + c0


@pytest.mark.parametrize("full,n", [((32, 32), 1024), ((32, 32), 896), ((28, 28), 784), ((16, 8, 8), 1024),
                                    ((10, 10, 8), 800), ((16, 16, 16), 4096), ((16, 16, 16), 3072)])
def test_arithmetic_index_equals_the_reference_buffer(full, n):
    want = ow.relative_position_index(full)[:n, :n]
    got = rel_index(full, n)
    assert got.min() >= 0 and got.max() < math.prod(2 * w - 1 for w in full)
    assert np.array_equal(got, want)
