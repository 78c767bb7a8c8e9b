"""Deferred augmentation on the host (long_context_biomedical_imaging_amd/data.py): drawing a transform chain's
parameters into a record and applying the record later gives bit for bit what the chain gives, with the same RNG
consumption; NumpyDataset(defer_aug=True) hands out those records; and the record layout agrees with include/lci.h.

The helpers below (records, the float64 nearest-neighbour rule) are shared with tests/test_augment_gpu.py."""
import ctypes
import os
import random
import re

import numpy as np
import pandas as pd
import pytest
import torch

from long_context_biomedical_imaging_amd import config as lconfig
from long_context_biomedical_imaging_amd import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 2.0 ** -10          # a coordinate further than this from a rounding tie decides its nearest index


# ------------------------------------------------------------------------------------------------ shared helpers
def make_row(seed, shape, affine=True, bc=False, blur=False):
    """One record with the recipes' draw ranges (define_transforms), the chosen flags forced on or off."""
    torch.manual_seed(seed)
    random.seed(seed)
    row = torch.zeros(data.AUG_FIELDS, dtype=torch.float64)
    m = data.RandomAffine(10, (0.1, 0.1), (0.95, 1.05), 10).draw(shape)
    alpha, beta = data.RandomBrightnessContrast().draw(shape)
    taps = data.GaussianBlur((1, 3), (0.1, 5)).draw(shape)[0]
    if affine:
        row[data.AUG_AFFINE_ON] = 1
        row[data.AUG_M:data.AUG_M + 6] = torch.tensor(m, dtype=torch.float32).double()
    if bc:
        row[data.AUG_BC_ON] = 1
        row[data.AUG_ALPHA], row[data.AUG_BETA] = alpha, beta
    if blur:
        row[data.AUG_BLUR_ON] = 1
        row[data.AUG_TAPS:data.AUG_TAPS + 3] = taps.double()
    return row


def source64(row, H, W):
    """The float64 rule for one record: (src, decided, cands). src (H, W) int64 is the flat source index of every
    output pixel (-1: the fill); decided (H, W) bool, the coordinate is more than DELTA from a tie on both axes;
    cands (4, H, W), the flat indices of the four adjacent source pixels (-1 outside the plane)."""
    ii, jj = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    if row[data.AUG_AFFINE_ON] == 0:
        src = (ii * W + jj).long()
        return src, torch.ones(H, W, dtype=torch.bool), src.expand(4, H, W)
    m = row[data.AUG_M:data.AUG_M + 6].float().double()
    xc, yc = jj - W / 2 + 0.5, ii - H / 2 + 0.5
    sx = m[0] * xc + m[1] * yc + m[2] + (W - 1) / 2
    sy = m[3] * xc + m[4] * yc + m[5] + (H - 1) / 2

    def flat(iy, ix):
        inside = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
        return torch.where(inside, iy * W + ix, torch.full_like(ix, -1)).long()

    decided = ((sx - sx.floor() - 0.5).abs() > DELTA) & ((sy - sy.floor() - 0.5).abs() > DELTA)
    fx, fy = sx.floor(), sy.floor()
    cands = torch.stack([flat(fy + dy, fx + dx) for dy in (0, 1) for dx in (0, 1)])
    return flat(torch.round(sy), torch.round(sx)), decided, cands        # torch.round: ties to even


def gather(x, src):
    """x (P, H, W) at the flat indices src (..., H, W), zero where src is -1."""
    flat = x.reshape(x.shape[0], -1)
    v = flat[:, src.clamp_min(0).reshape(-1)].reshape(x.shape[0], *src.shape)
    return torch.where(src >= 0, v, torch.zeros((), dtype=x.dtype))


def check_nearest(y, x, row, what=""):
    """The comparison rule for an affine-only result y of x (P, H, W) under `row`: the oracle's source pixel
    wherever it is decided, one of the adjacent candidates or the fill elsewhere. Returns the shares (undecided,
    inside the plane)."""
    P, H, W = x.shape
    src, decided, cands = source64(row, H, W)
    want = gather(x, src)
    bad = decided & (y != want).any(0)
    assert not bad.any(), f"{what}: {int(bad.sum())} decided pixels differ from the oracle's source pixel"
    near = (gather(x, cands) == y[:, None]).any(1) | (y == 0)
    assert near[:, ~decided].all(), f"{what}: an undecided pixel holds neither an adjacent candidate nor the fill"
    return 1.0 - decided.double().mean().item(), (src >= 0).double().mean().item()


def write_dataset(tmp, n, shape, task, seed=1):
    rng = np.random.default_rng(seed)
    for i in range(n):
        d = tmp / f"s{i:02d}"
        d.mkdir()
        np.save(d / f"s{i:02d}_input.npy", rng.standard_normal(shape).astype(np.float32))
        if task == "seg":
            np.save(d / f"s{i:02d}_output.npy", rng.integers(0, 3, shape).astype(np.float32))
        elif task == "enhance":
            np.save(d / f"s{i:02d}_output.npy", rng.standard_normal(shape).astype(np.float32))
    if task == "class":
        ids = [f"s{i:02d}" for i in range(n)]
        pd.DataFrame({"SubjectID": ids, "Label": [i % 3 for i in range(n)]}).to_csv(tmp / "x_metadata.csv",
                                                                                  index=False)


def dataset_config(tmp, task, hw=(16, 16), time=1, *extra):
    return lconfig.parse_config(["--data_dir", str(tmp), "--height", str(hw[0]), "--width", str(hw[1]), "--time",
                                 str(time), "--no_out_channel", "3" if task == "seg" else "1", "--task_type", task,
                                 *extra])


# --------------------------------------------------------------------------------------------------------- tests
COMBOS = [(task, bc, blur) for task in ("seg", "enhance", "class") for bc in (True, False) for blur in (True, False)]


@pytest.mark.parametrize("task,bc,blur", COMBOS)
def test_draw_then_apply_is_the_chain_bitwise(task, bc, blur, tmp_path):
    cfg = dataset_config(tmp_path, task, (16, 16), 1, "--brightness_aug", str(bc), "--gaussian_blur_aug", str(blur))
    seen = set()
    for seed in range(12):
        for which, chain in enumerate(data.define_transforms(cfg, "train")):
            img = torch.randn(2, 3, 17, 23, generator=torch.Generator().manual_seed(100 + seed))
            random.seed(seed)
            torch.manual_seed(seed)
            want = chain(img)
            state = (torch.get_rng_state(), random.getstate())
            random.seed(seed)
            torch.manual_seed(seed)
            row = data.draw_params(chain, img.shape)
            assert torch.equal(torch.get_rng_state(), state[0]) and random.getstate() == state[1]
            assert row.dtype == torch.float64 and tuple(row.shape) == (data.AUG_FIELDS,)
            got = data.apply_params(img, row)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (seed, which)
            f32 = torch.cat([row[data.AUG_M:data.AUG_M + 6], row[data.AUG_TAPS:data.AUG_TAPS + 3]])
            assert torch.equal(f32.float().double(), f32)            # m and taps are already f32 values
            if which == 0:
                seen.add(tuple(int(row[f]) for f in data.AUG_FLAGS))
            else:                                                    # the target chain never blurs
                assert row[data.AUG_BLUR_ON] == 0 and (task == "enhance" or row[data.AUG_BC_ON] == 0)
    assert (1, int(bc), 0) in seen                                   # the common draw did occur
    assert all(f[1] <= int(bc) and f[2] <= int(blur) for f in seen)


def test_val_chain_draws_nothing(tmp_path):
    cfg = dataset_config(tmp_path, "seg")
    for chain in data.define_transforms(cfg, "val"):
        torch.manual_seed(3)
        state = torch.get_rng_state()
        assert not data.draw_params(chain, (1, 1, 16, 16)).any()
        assert torch.equal(torch.get_rng_state(), state)


def test_draw_params_refuses_other_chains():
    blur, aff = data.GaussianBlur((1, 3), (0.1, 5)), data.RandomAffine(10)
    with pytest.raises(ValueError, match="order"):
        data.draw_params(data.Compose([data.RandomApply([blur], 1.0), data.RandomApply([aff], 1.0)]), (1, 8, 8))
    with pytest.raises(ValueError, match="kernel_size"):
        data.draw_params(data.Compose([data.RandomApply([data.GaussianBlur((3, 3), (0.1, 5))], 1.0)]), (1, 8, 8))
    with pytest.raises(ValueError, match="RandomApply"):
        data.draw_params(data.Compose([aff]), (1, 8, 8))


@pytest.mark.parametrize("task", ["seg", "enhance", "class"])
def test_deferred_dataset_reproduces_the_default(task, tmp_path):
    write_dataset(tmp_path, 5, (16, 16, 4), task)
    cfg = dataset_config(tmp_path, task, (16, 16), 4)
    plain, deferred = data.NumpyDataset(cfg, "train"), data.NumpyDataset(cfg, "train", defer_aug=True)
    assert len(plain) == len(deferred) == 3
    flags = set()
    for rep in range(6):
        for i in range(len(plain)):
            np.random.seed(10 * rep + i)
            item = plain[i]
            assert len(item) == 3                                    # the default item is unchanged
            np.random.seed(10 * rep + i)
            img, tgt, sid, params = deferred[i]
            assert sid == item[2] and tuple(params.shape) == (2, data.AUG_FIELDS) and params.dtype == torch.float64
            assert torch.equal(data.apply_params(img, params[0]), item[0])
            flags.add(tuple(int(params[0, f]) for f in data.AUG_FLAGS))
            if task == "class":
                assert torch.equal(tgt, item[1]) and not params[1].any()
                continue
            assert tgt.dtype == item[1].dtype and tgt.shape == item[1].shape
            assert torch.equal(data.apply_params(tgt, params[1]), item[1])
            aff = slice(data.AUG_AFFINE_ON, data.AUG_M + 6)
            assert torch.equal(params[0, aff], params[1, aff])       # image and target share one affine
            if task == "seg":
                raw = np.load(tmp_path / sid / f"{sid}_output.npy")
                assert torch.equal(tgt, torch.from_numpy(raw).permute(2, 0, 1).long())   # un-augmented (T, H, W)
                assert not params[1, data.AUG_M + 6:].any()
    assert len(flags) > 1                                            # the draws differ from item to item
    batch = next(iter(torch.utils.data.DataLoader(deferred, batch_size=3)))
    assert tuple(batch[3].shape) == (3, 2, data.AUG_FIELDS)
    for split in ("val", "test"):
        item = data.NumpyDataset(cfg, split, defer_aug=True)[0]
        assert len(item) == 4 and not item[3].any()
        ref = data.NumpyDataset(cfg, split)[0]
        assert torch.equal(item[0], ref[0]) and torch.equal(item[1], ref[1])


def test_record_layout_matches_the_header():
    """Taps sum to 1; data.AUG_* are the indices include/lci.h lists for lci_augment's params."""
    for seed in range(12):
        row = make_row(seed, (1, 8, 8), blur=True)
        assert abs(row[data.AUG_TAPS:data.AUG_TAPS + 3].sum().item() - 1.0) < 1e-6
    txt = open(os.path.join(ROOT, "include", "lci.h")).read()
    sec = txt[txt.index("params : (B, 16) f32"):txt.index("Per sample, with w the warped sample")]
    table = {}
    for first, last, names in re.findall(r"^ \*\s+(\d+)(?:(?:\.\.|, )(\d+))?\s+([a-z_]+(?:\[[^\]]*\])?(?:, [a-z_]+)?)",
                                         sec, flags=re.M):
        table[names] = (int(first), int(last or first))
    assert table == {"affine_on": (data.AUG_AFFINE_ON,) * 2, "m[0..5]": (data.AUG_M, data.AUG_M + 5),
                     "bc_on": (data.AUG_BC_ON,) * 2, "alpha, beta": (data.AUG_ALPHA, data.AUG_BETA),
                     "blur_on": (data.AUG_BLUR_ON,) * 2, "taps[0..2]": (data.AUG_TAPS, data.AUG_TAPS + 2),
                     "zero": (14, data.AUG_FIELDS - 1)}
    assert data.AUG_FIELDS == 16


def test_abi_declares_augment():
    from long_context_biomedical_imaging_amd import _lib, kernels
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    version, sigs = _lib.header()
    assert version >= 40
    assert sigs["lci_augment"] == (I, [P, P, I, P, P, I, I, I, I, P])
    assert sigs["lci_augment_ws_bytes"] == (L, [I, I, I, I])
    assert kernels.AUG_FIELDS == data.AUG_FIELDS


def test_float64_rule_agrees_with_the_host_path():
    """The host path (f32 grid_sample) picks the float64 rule's source pixel on every decided pixel, and the inputs
    the GPU tests use keep their conditions: at most 2 % undecided, at least 60 % inside the plane."""
    for shape in [(3, 37, 53), (1, 64, 48), (2, 19, 130)]:
        for seed in range(12):
            row = make_row(seed, shape)
            x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
            und, inside = check_nearest(data.apply_params(x, row), x, row, f"{shape} seed {seed}")
            assert und <= 0.02 and inside >= 0.60, (shape, seed, und, inside)
