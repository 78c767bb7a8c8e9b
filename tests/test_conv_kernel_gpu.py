"""GPU: every kernel of the decoder-head convolution (csrc/conv.hip) called through the C entry points lci_conv3_fwd,
lci_conv3_fwd_split (with an explicit nsplit) and lci_conv3_wgrad on caller-owned buffers, against plain fp64 sums over
taps written here (_reference, _reference_dgrad, _reference_wgrad), per element. The three are pinned once, on the CPU,
against F.conv3d / F.conv2d with autograd in fp64 (tests/test_conv_cpu.py, not a GPU test).

Conventions restated here, independently of torch: tap = (kd * 3 + kh) * 3 + kw reads the voxel at offset
(kd - 1, kh - 1, kw - 1) (zero outside the volume; KD = 1: kd is fixed at 1); the forward kernels reduce over slabs
sl = grp * (Cin / 32) + chunk, grp = tap // 3 (the three kw taps of a (kd, kh) row and one 32-channel chunk), and
split s of nsplit owns the slabs [nslab s // nsplit, nslab (s + 1) // nsplit); the weight gradient enumerates voxels
as gapped rows,
one gap row after every line of W voxels (R = (V / W)(W + 1) rows), and split s of ns owns the rows [s Lv, (s + 1) Lv)
with Lv = roundup(ceil(R / ns), 128). The packed weight (Cout, T, Cin) is built with permute, not with
lci_conv3_pack_weight (which test_conv_gpu.py checks bit for bit).

Inputs, one seeded CPU generator per case: x, dy ~ N(0, 1), w ~ N(0, 1) / sqrt(T Cin), each rounded to bf16 before
either side sees it. Every buffer is a view inside a larger allocation with 64-element guard bands on both sides. The
guards of the inputs x, w, dy hold NaN: the zero rows the DMA kernels read before row 0 and past row V then come from
the buffer resource's bounds alone, and any unmasked out-of-range read turns into a NaN of the output. The outputs (y,
the forward partials, the weight-gradient partials) are pre-filled with NaN and must come out finite everywhere, with
their guard bands bitwise untouched.

Forward cases, unsplit (lci_conv3_fwd); V = B D H W voxels in blocks of 512 (8 waves of 64):
  lds2_32_32       32 -> 32, 2 x (5, 7, 9): conv3_fwd_lds2_kernel<1>; V = 630: a second block of 118 voxels (a half-live
                   wave, dead waves), the sample seam at voxel 315 inside block 0
  lds2_2d          64 -> 32, 1 x (1, 19, 31): lds2<1> with 9 taps, two channel chunks
  lds2_160         32 -> 160, 1 x (3, 6, 7): lds2<1> in order 1, ntile 5, the grid padded 5 -> 8 (three workgroups
                   return)
  dma2             64 -> 64, 2 x (4, 9, 11): conv3_fwd_dma_kernel<2, false>, order 0, ragged tail (V = 792)
  dma3             96 -> 96, 3 x (3, 5, 13): dma<3, false>, order 1, three samples within two blocks
  dma3_192         32 -> 192, 1 x (9, 10, 11): dma<3, false>, two Cout tiles
  dma4             64 -> 128, 2 x (6, 6, 6): dma<4, false> (SPREAD); V = 432: wave 7 is not live (its `!live` issue
                   path)
  dma4_256         128 -> 256, 2 x (5, 7, 9): dma<4, false>, two tiles, four chunks
  tiny_h1          32 -> 64, 3 x (2, 1, 3): V = 18 < 32, H = 1
  tiny_d1          32 -> 64, 2 x (1, 5, 1) with KD = 3: W = 1, D = 1 under 27 taps
  vec1 .. vec4     16 -> 32, 80 -> 64 (2-D, 1 x (1, 19, 31)), 48 -> 96, 16 -> 128 at 2 x (5, 7, 9):
                   conv3_fwd_kernel<NT, 4>, NT = 1, 2, 3, 4
  gen3, gen4, gen1 1 -> 96, 5 -> 128, 24 -> 32 at 1 x (8, 9, 10); gen2_2d 3 -> 64 at 1 x (1, 20, 24):
                   conv3_fwd_generic_kernel<NT>, K padded to 16
  dgrad            the data gradient of a 40 -> 64 conv at 2 x (4, 9, 11): dx = conv(dy, w') with w'[c, t, n] =
                   w[n, c, T - 1 - t] zero-padded to (64, T, 64), built in torch (dma<2, false>); dx[..., :40] against
                   the fp64 adjoint (a scatter over taps, not the flipped conv), dx[..., 40:] exactly zero
Forward cases, split (lci_conv3_fwd_split: conv3_fwd_dma_kernel<NT, true> + conv3_sum_kernel):
  split2           32 -> 32, 2 x (5, 7, 9), nsplit 2: slab ranges of 4 and 5
  split9           the same, nsplit 9: one slab per split (a single loop pass, nothing issued ahead)
  split4_96        96 -> 96, 3 x (3, 5, 13), nsplit 4: 27 slabs as 6 / 7 / 7 / 7, seams inside a tap group
  split3_2d        64 -> 128, 2 x (1, 19, 31), nsplit 3: 6 slabs
  split2_zero      64 -> 64, 2 x (4, 9, 11), nsplit 2, weight rows 40..63 zero: those outputs and partials exactly zero
Weight-gradient cases (lci_conv3_wgrad; WGRAD), each (Cin -> Cout) at 2 x (9, 7, 13) (V = 1638, ns >= 2 asserted) and at
the 2-D 1 x (1, 70, 50); both have ragged lines and more than two 128-row steps per split:
  32 -> 32, 32 -> 96        conv3_wgrad4_kernel<1>
  64 -> 64, 96 -> 64        conv3_wgrad4_kernel<2>
  128 -> 128                conv3_wgrad5_kernel<2, 2, 4>
  64 -> 128                 conv3_wgrad5_kernel<2, 2, 2>
  96 -> 96                  conv3_wgrad6_kernel<3>, and conv3_wgrad5_kernel<1, 3, 3> with LCI_WGRAD_DMA=0
  64 -> 96                  conv3_wgrad6_kernel<2>, and conv3_wgrad5_kernel<1, 3, 2> with LCI_WGRAD_DMA=0
  tiny: 32 -> 32 at 3 x (2, 1, 3) and at 2 x (1, 5, 1) with KD = 3
  empty: 2 x (25, 77, 3) at 32 -> 32 (v4) and 96 -> 96 (v6, v5): 3850 lines, V = 11550, R = 15400, ns = 12, Lv = 1408,
  11 x 1408 = 15488 >= R: the last split owns no row and must write zeros (the caller sums every split of a
  torch.empty workspace). That the last split is empty is asserted from the restated arithmetic on the device's ns.

Bounds, all against fp64 on the same bf16-rounded operands and per element:
  f32 outputs (each forward partial against the fp64 sum of its slabs, each weight-gradient partial against the fp64
  sum over its voxels, and the fp64 sum of the partials against the whole): |err| <= 1e-4 max|ref| + 1e-6, max|ref| over
  that tensor (the bound of test_conv3_wgrad_dma_vs_register_staging)
  bf16 y: |err| <= 2^-8 |ref| + 1e-4 max|ref| (test_scan_kernel_gpu.py's rule for one bf16 rounding of an f32 value)
  where the reference is identically zero (zero weight rows, padded data-gradient channels, the empty split) the result
  is exactly zero
Exact checks: the split forward's y equals bf16(((0 + p0) + p1) + ...) of the partials the kernel wrote, added in f32 in
split order with torch, bit for bit (conv3_sum_kernel judged apart from the MFMA kernel); the last sample repacked as a
B = 1 problem gives that sample's y (and partials) bit for bit; two runs over differently pre-filled outputs (NaN, 3.0)
agree bit for bit, forward and weight gradient; the (1, 3, WC) weight gradients with LCI_WGRAD_DMA=0 equal the default
bit for bit. Host checks: Cout = 48, KD = 2, KD = 1 with D = 2, an x pointer offset by 8 bytes, split with Cin = 16,
split with a null workspace, nsplit above the slab count (10 > 9) and a weight gradient with Cin = 16 each raise
LciError and leave the NaN-pre-filled outputs untouched. lci_conv3_fwd_splits is compared with a restatement of its
rule on the CPU (tests/test_conv_cpu.py).

Measured on an MI355X: the largest per-element error of each case as a fraction of its allowance (y: the bf16 output;
part: the worst f32 partial; sum: the fp64 sum of the partials; rnd: what the bf16 rounding of the exact fp64 value
alone gives against y's allowance, computed on the CPU: y equals it to two digits, so the kernels add nothing visible
to that rounding; the f32 outputs sit at 0.1 - 0.6 % of theirs). Every exact check held bit for bit.
case               y   part    sum    rnd   (forward; part / sum: split cases only)
lds2_32_32      0.92      -      -   0.92
lds2_2d         0.94      -      -   0.94
lds2_160        0.93      -      -   0.93
dma2            0.94      -      -   0.94
dma3            0.94      -      -   0.94
dma3_192        0.94      -      -   0.94
dma4            0.94      -      -   0.94
dma4_256        0.94      -      -   0.94
tiny_h1         0.93      -      -   0.93
tiny_d1         0.88      -      -   0.88
vec1            0.94      -      -   0.94
vec2_2d         0.92      -      -   0.92
vec3            0.94      -      -   0.94
vec4            0.94      -      -   0.94
gen3            0.93      -      -   0.93
gen4            0.94      -      -   0.94
gen1            0.95      -      -   0.95
gen2_2d         0.94      -      -   0.94
dgrad           0.92      -      -   0.92
split2          0.93  0.004  0.003   0.93
split9          0.94  0.001  0.001   0.94
split4_96       0.94  0.004  0.002   0.94
split3_2d       0.93  0.002  0.001   0.93
split2_zero     0.93  0.003  0.003   0.93
case           ns   part    sum   (weight gradient; with LCI_WGRAD_DMA=0 bitwise the same)
32_32_3d        2  0.001  0.001
32_32_2d        4  0.002  0.001
32_96_3d        2  0.001  0.001
32_96_2d        4  0.001  0.001
64_64_3d        2  0.001  0.001
64_64_2d        4  0.002  0.001
96_64_3d        2  0.001  0.001
96_64_2d        4  0.001  0.001
128_128_3d      2  0.004  0.003
128_128_2d      4  0.004  0.003
64_128_3d       2  0.004  0.003
64_128_2d       4  0.005  0.003
96_96_3d        2  0.004  0.003
96_96_2d        4  0.004  0.003
64_96_3d        2  0.004  0.003
64_96_2d        4  0.005  0.003
tiny_h1         1  0.001  0.001
tiny_d1         1  0.000  0.000
empty_32_32    12  0.002  0.001
empty_96_96    12  0.006  0.002
"""
import dataclasses
import functools
import math
import os

import pytest
import torch

gpu = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64            # guard-band elements on either side (128 B of bf16, 256 B of f32: keeps the 16-byte alignment)
SENTINEL = -7.0       # exact in bf16 and f32
U_BF16 = 2.0 ** -8
FILLS = {"nan": float("nan"), "three": 3.0}
WG_ROWS = 128         # csrc/conv.hip WG_ROWS


@dataclasses.dataclass(frozen=True)
class Fwd:
    Cin: int
    Cout: int
    B: int
    S: tuple                   # (D, H, W)
    KD: int = 0                # 0: 3, or 1 when D == 1
    nsplit: int = 0            # 0: lci_conv3_fwd; else lci_conv3_fwd_split with this nsplit
    zero_from: int = 0         # output channels [zero_from, Cout) have zero weight rows (0: none)
    dgrad_cin: int = 0         # the data-gradient form of a (dgrad_cin -> Cin) conv; Cout is dgrad_cin padded to 32

    @property
    def kd(self):
        return self.KD or (1 if self.S[0] == 1 else 3)

    @property
    def V(self):
        return self.B * math.prod(self.S)


FWD = {
    "lds2_32_32": Fwd(32, 32, 2, (5, 7, 9)),
    "lds2_2d": Fwd(64, 32, 1, (1, 19, 31)),
    "lds2_160": Fwd(32, 160, 1, (3, 6, 7)),
    "dma2": Fwd(64, 64, 2, (4, 9, 11)),
    "dma3": Fwd(96, 96, 3, (3, 5, 13)),
    "dma3_192": Fwd(32, 192, 1, (9, 10, 11)),
    "dma4": Fwd(64, 128, 2, (6, 6, 6)),
    "dma4_256": Fwd(128, 256, 2, (5, 7, 9)),
    "tiny_h1": Fwd(32, 64, 3, (2, 1, 3)),
    "tiny_d1": Fwd(32, 64, 2, (1, 5, 1), KD=3),
    "vec1": Fwd(16, 32, 2, (5, 7, 9)),
    "vec2_2d": Fwd(80, 64, 1, (1, 19, 31)),
    "vec3": Fwd(48, 96, 2, (5, 7, 9)),
    "vec4": Fwd(16, 128, 2, (5, 7, 9)),
    "gen3": Fwd(1, 96, 1, (8, 9, 10)),
    "gen4": Fwd(5, 128, 1, (8, 9, 10)),
    "gen1": Fwd(24, 32, 1, (8, 9, 10)),
    "gen2_2d": Fwd(3, 64, 1, (1, 20, 24)),
    "dgrad": Fwd(64, 64, 2, (4, 9, 11), zero_from=40, dgrad_cin=40),
    "split2": Fwd(32, 32, 2, (5, 7, 9), nsplit=2),
    "split9": Fwd(32, 32, 2, (5, 7, 9), nsplit=9),
    "split4_96": Fwd(96, 96, 3, (3, 5, 13), nsplit=4),
    "split3_2d": Fwd(64, 128, 2, (1, 19, 31), nsplit=3),
    "split2_zero": Fwd(64, 64, 2, (4, 9, 11), nsplit=2, zero_from=40),
}


@dataclasses.dataclass(frozen=True)
class Wg:
    Cin: int
    Cout: int
    B: int
    S: tuple
    KD: int = 0
    v5_too: bool = False       # a (1, 3, WC) tile: also run with LCI_WGRAD_DMA=0
    min_ns: int = 1
    empty_last: bool = False   # the last voxel split owns no row

    kd = Fwd.kd
    V = Fwd.V


WGRAD = {}
for _ci, _co in ((32, 32), (32, 96), (64, 64), (96, 64), (128, 128), (64, 128), (96, 96), (64, 96)):
    _v5 = _co == 96 and _ci != 32
    WGRAD[f"{_ci}_{_co}_3d"] = Wg(_ci, _co, 2, (9, 7, 13), v5_too=_v5, min_ns=2)
    WGRAD[f"{_ci}_{_co}_2d"] = Wg(_ci, _co, 1, (1, 70, 50), v5_too=_v5)
WGRAD["tiny_h1"] = Wg(32, 32, 3, (2, 1, 3))
WGRAD["tiny_d1"] = Wg(32, 32, 2, (1, 5, 1), KD=3)
WGRAD["empty_32_32"] = Wg(32, 32, 2, (25, 77, 3), empty_last=True)
WGRAD["empty_96_96"] = Wg(96, 96, 2, (25, 77, 3), v5_too=True, empty_last=True)


# ------------------------------------------------------------------------------------------------ fp64 side (CPU)
def _taps(KD):
    """(tap, kd, kh, kw) in the kernels' tap order; the voxel read is at offset (kd - 1, kh - 1, kw - 1)."""
    return [((kd * 3 + kh) * 3 + kw if KD == 3 else kh * 3 + kw, kd, kh, kw)
            for kd in (range(3) if KD == 3 else (1,)) for kh in range(3) for kw in range(3)]


def _shifted(x, kd, kh, kw):
    """x (B, D, H, W, C) -> the same shape, voxel p holding x[p + (kd - 1, kh - 1, kw - 1)], zero outside the volume."""
    B, D, H, W, C = x.shape
    xp = x.new_zeros(B, D + 2, H + 2, W + 2, C)
    xp[:, 1:D + 1, 1:H + 1, 1:W + 1] = x
    return xp[:, kd:kd + D, kh:kh + H, kw:kw + W]


def _reference(x, w, KD, slabs=False):
    """y[b, p, n] = sum over taps and channels of x[b, p + off(tap), c] w[n, c, tap] in fp64: x (B, D, H, W, Cin),
    w (Cout, Cin, T). With slabs = True also the contribution (nslab, B, D, H, W, Cout) of every slab
    sl = (tap // 3) * (Cin / 32) + chunk."""
    x, w = x.double(), w.double()
    Cout, Cin, T = w.shape
    assert T == KD * 9
    nch = Cin // 32
    y = x.new_zeros(*x.shape[:4], Cout)
    per = x.new_zeros(KD * 3 * nch, *x.shape[:4], Cout) if slabs else None
    for tap, kd, kh, kw in _taps(KD):
        xs = _shifted(x, kd, kh, kw)
        y += xs @ w[:, :, tap].T
        for ch in range(nch if slabs else 0):
            c = slice(32 * ch, 32 * ch + 32)
            per[(tap // 3) * nch + ch] += xs[..., c] @ w[:, c, tap].T
    return (y, per) if slabs else y


def _reference_dgrad(dy, w, KD):
    """dx of _reference, as its adjoint: voxel p's dy scattered to p + off(tap) through w[:, :, tap]. dy (B, D, H, W,
    Cout), w (Cout, Cin, T) -> (B, D, H, W, Cin)."""
    dy, w = dy.double(), w.double()
    B, D, H, W, _ = dy.shape
    dxp = dy.new_zeros(B, D + 2, H + 2, W + 2, w.shape[1])
    for tap, kd, kh, kw in _taps(KD):
        dxp[:, kd:kd + D, kh:kh + H, kw:kw + W] += dy @ w[:, :, tap]
    return dxp[:, 1:D + 1, 1:H + 1, 1:W + 1].contiguous()


def _wgrad_split_of_voxel(V, W, Lv):
    """The voxel split of every voxel: voxel p of line p // W is gapped row (p // W)(W + 1) + p % W."""
    p = torch.arange(V)
    return ((p // W) * (W + 1) + p % W) // Lv


def _reference_wgrad(x, dy, KD, ns, Lv):
    """(ns, T, Cout, Cin) fp64: split s holds sum over its voxels p of dy[p, n] x[p + off(tap), c]."""
    x, dy = x.double(), dy.double()
    B, D, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    sid = _wgrad_split_of_voxel(B * D * H * W, W, Lv)
    out = x.new_zeros(ns, KD * 9, Cout, Cin)
    dyf = dy.reshape(-1, Cout)
    for tap, kd, kh, kw in _taps(KD):
        xs = _shifted(x, kd, kh, kw).reshape(-1, Cin)
        for s in range(ns):
            m = sid == s
            if m.any():
                out[s, tap] = dyf[m].T @ xs[m]
    return out


def _nt(Cout):
    nb = Cout // 32
    return 3 if nb % 3 == 0 else (4 if nb % 4 == 0 else (2 if nb % 2 == 0 else 1))


def _expected_fwd_splits(V, Cin, Cout, KD):
    """lci_conv3_fwd_splits's rule: under 256 workgroups of 512 voxels x 32 NT channels, about 512 workgroups, at least
    two slabs per split, at most 64 splits and 100 MB of f32 partials."""
    if V <= 0 or Cin % 32 or Cout % 32 or KD not in (1, 3):
        return 1
    nb = -(-V // 512) * (Cout // (32 * _nt(Cout)))
    if nb >= 256:
        return 1
    s = min(-(-512 // nb), KD * 3 * (Cin // 32) // 2, 64)
    while s > 1 and s * V * Cout * 4 > (100 << 20):
        s -= 1
    return max(s, 1)


def _wgrad_rows(V, W, ns):
    """(R, Lv) of lci_conv3_wgrad for ns voxel splits."""
    R = (V // W) * (W + 1)
    return R, -(-(-(-R // ns)) // WG_ROWS) * WG_ROWS


def _randn_bf16(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16).float()


@functools.lru_cache(maxsize=None)
def _fwd_inputs(name):
    """x (B, D, H, W, Cin), the packed weight wp (Cout, T, Cin) the kernel reads, and the (Cout, Cin, T) weight the
    reference reads (dgrad: the original conv's (Cin, dgrad_cin, T) weight), all holding bf16 values."""
    c = FWD[name]
    g = torch.Generator().manual_seed(9000 + list(FWD).index(name))
    T = c.kd * 9
    x = _randn_bf16(g, c.B, *c.S, c.Cin)
    if c.dgrad_cin:   # x is dy (.., Cin = the conv's output channels); w0 the conv's weight (n, c, tap)
        w0 = _randn_bf16(g, c.Cin, c.dgrad_cin, T, scale=(T * c.dgrad_cin) ** -0.5)
        wp = torch.zeros(c.Cout, T, c.Cin)
        wp[:c.dgrad_cin] = w0.flip(2).permute(1, 2, 0)         # w'[c, t, n] = w0[n, c, T - 1 - t]
        return x, wp, w0
    w = _randn_bf16(g, c.Cout, c.Cin, T, scale=(T * c.Cin) ** -0.5)
    if c.zero_from:
        w[c.zero_from:] = 0.0
    return x, w.permute(0, 2, 1).contiguous(), w


@functools.lru_cache(maxsize=None)
def _fwd_ref(name):
    """(y (V, Cout), per-split partial sums (nsplit, V, Cout) or None) in fp64; computed once, never modified."""
    c = FWD[name]
    x, _, w = _fwd_inputs(name)
    if c.dgrad_cin:
        dx = _reference_dgrad(x, w, c.kd)
        y = torch.cat([dx, dx.new_zeros(*dx.shape[:4], c.Cout - c.dgrad_cin)], -1)
        return y.reshape(c.V, c.Cout), None
    if not c.nsplit:
        return _reference(x, w, c.kd).reshape(c.V, c.Cout), None
    y, per = _reference(x, w, c.kd, slabs=True)
    nslab = per.shape[0]
    parts = torch.stack([per[nslab * s // c.nsplit:nslab * (s + 1) // c.nsplit].sum(0) for s in range(c.nsplit)])
    return y.reshape(c.V, c.Cout), parts.reshape(c.nsplit, c.V, c.Cout)


@functools.lru_cache(maxsize=None)
def _wg_inputs(name):
    c = WGRAD[name]
    g = torch.Generator().manual_seed(9500 + list(WGRAD).index(name))
    return _randn_bf16(g, c.B, *c.S, c.Cin), _randn_bf16(g, c.B, *c.S, c.Cout)


@functools.lru_cache(maxsize=None)
def _wg_ref(name, ns):
    c = WGRAD[name]
    x, dy = _wg_inputs(name)
    return _reference_wgrad(x, dy, c.kd, ns, _wgrad_rows(c.V, c.S[2], ns)[1])


# ------------------------------------------------------------------------------------------------ device side
def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


class _In:
    """A CPU tensor on the device as a contiguous view inside a flat buffer whose guard bands hold NaN."""

    def __init__(self, t, dtype=BF16):
        n = t.numel()
        self.flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.view = self.flat[GUARD:GUARD + n].view(t.shape)
        self.view.copy_(t)

    def ptr(self):
        return self.view.data_ptr()


class _Out:
    """An output of `shape` inside a flat buffer: sentinel guard bands on both sides, the view pre-filled by `fill`."""

    def __init__(self, shape, dtype, fill):
        n = math.prod(shape)
        self.flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.flat[GUARD:GUARD + n].view(shape)
        self.view.fill_(fill)
        self.before = self.flat.clone()

    def guards_intact(self):
        a, b = _bits(self.flat), _bits(self.before)
        return torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:])

    def unchanged(self):
        return torch.equal(_bits(self.flat), _bits(self.before))

    def ptr(self):
        return self.view.data_ptr()


def _launch_fwd(x, wp, KD, nsplit, fill, bad=None):
    """lci_conv3_fwd (nsplit 0) or lci_conv3_fwd_split on fresh guarded buffers. `bad` (host-check tests) replaces
    arguments by invalid ones; the call is then expected to raise before anything is launched."""
    from long_context_biomedical_imaging_amd import _lib
    bad = bad or {}
    B, D, H, W, Cin = x.shape
    Cout, V = wp.shape[0], B * D * H * W
    xd, wd = _In(x), _In(wp)
    y = _Out((V, Cout), BF16, fill)
    part = _Out((max(nsplit, 1), V, Cout), F32, fill)
    dims = (B, bad.get("D", D), H, W, bad.get("Cin", Cin), bad.get("Cout", Cout), bad.get("KD", KD))
    xptr, stream = xd.ptr() + bad.get("x_offset", 0), _lib.stream_of(xd.view)
    if nsplit:
        run = lambda: _lib.call("lci_conv3_fwd_split", xptr, wd.ptr(), y.ptr(),  # noqa: E731
                                None if bad.get("null_part") else part.ptr(), nsplit, *dims, stream)
    else:
        run = lambda: _lib.call("lci_conv3_fwd", xptr, wd.ptr(), y.ptr(), *dims, stream)  # noqa: E731
    if bad:
        with pytest.raises(_lib.LciError):
            run()
        torch.cuda.synchronize()
        return y.unchanged() and part.unchanged()
    run()
    torch.cuda.synchronize()
    return dict(y=y.view.cpu(), part=part.view.cpu() if nsplit else None,
                intact=y.guards_intact() and (part.guards_intact() if nsplit else part.unchanged()))


@functools.lru_cache(maxsize=None)
def _run_fwd(name, fill="nan", sample=None):
    c = FWD[name]
    x, wp, _ = _fwd_inputs(name)
    if sample is not None:
        x = x[sample:sample + 1]
    return _launch_fwd(x, wp, c.kd, c.nsplit, FILLS[fill])


def _launch_wgrad(x, dy, KD, fill, bad=None):
    from long_context_biomedical_imaging_amd import _lib
    bad = bad or {}
    B, D, H, W, Cin = x.shape
    Cout, V = dy.shape[-1], B * D * H * W
    ns = int(_lib.load().lci_conv3_wgrad_splits(V, Cin, Cout, KD))
    xd, dyd = _In(x), _In(dy)
    part = _Out((ns, KD * 9, Cout, Cin), F32, fill)
    run = lambda: _lib.call("lci_conv3_wgrad", xd.ptr(), dyd.ptr(), part.ptr(), B, D, H, W,  # noqa: E731
                            bad.get("Cin", Cin), Cout, KD, _lib.stream_of(xd.view))
    if bad:
        with pytest.raises(_lib.LciError):
            run()
        torch.cuda.synchronize()
        return part.unchanged()
    run()
    torch.cuda.synchronize()
    return dict(part=part.view.cpu(), ns=ns, intact=part.guards_intact())


@functools.lru_cache(maxsize=None)
def _run_wgrad(name, fill="nan", dma=True):
    """dma = False: the caller has set LCI_WGRAD_DMA=0 (the library reads it per call)."""
    assert (os.environ.get("LCI_WGRAD_DMA") == "0") == (not dma)
    c = WGRAD[name]
    x, dy = _wg_inputs(name)
    return _launch_wgrad(x, dy, c.kd, FILLS[fill])


# ------------------------------------------------------------------------------------------------ metrics
def _frac_f32(x, ref):
    """Largest |err| / (1e-4 max|ref| + 1e-6); a NaN gives inf."""
    err = (x.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    return (err.max() / (1e-4 * ref.abs().max() + 1e-6)).item()


def _frac_bf16(x, ref):
    """Largest |err| / (2^-8 |ref| + 1e-4 max|ref|); with no allowance (an all-zero reference) exact or inf."""
    err = (x.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    allowed = U_BF16 * ref.abs() + 1e-4 * ref.abs().max()
    if (err[allowed == 0] != 0).any():
        return math.inf
    return (err / allowed.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------------------------------------ tests
@gpu
@pytest.mark.parametrize("name", list(FWD))
def test_conv_fwd_vs_fp64(name):
    """y (and with a split every f32 partial and their sum) per element against the fp64 sum over taps, with the
    pre-fill, guard-band, exact-zero and split-sum checks of the module docstring."""
    c, out = FWD[name], _run_fwd(name)
    yref, pref = _fwd_ref(name)
    y, fails = out["y"], []
    if not out["intact"]:
        fails.append("guard band of y or of the partials written")
    if not torch.isfinite(y).all():
        fails.append("y: non-finite entries left")
    live = slice(0, c.zero_from or c.Cout)
    fy = _frac_bf16(y[:, live], yref[:, live])
    rnd = _frac_bf16(yref.to(BF16)[:, live], yref[:, live])
    if not fy <= 1.0:
        fails.append(f"y: per-element error {fy:.3f} x the allowance")
    if c.zero_from and (yref[:, c.zero_from:].any() or _bits(y[:, c.zero_from:].contiguous()).any()):
        fails.append("y: nonzero where the reference is identically zero")
    fp = fs = float("nan")
    if c.nsplit:
        part = out["part"]
        if not torch.isfinite(part).all():
            fails.append("partials: non-finite entries left")
        fp = max(_frac_f32(part[s][:, live], pref[s][:, live]) for s in range(c.nsplit))
        fs = _frac_f32(part.double().sum(0)[:, live], yref[:, live])
        if not fp <= 1.0:
            fails.append(f"partials: per-element error {fp:.3f} x the allowance")
        if not fs <= 1.0:
            fails.append(f"sum of the partials: per-element error {fs:.3f} x the allowance")
        if c.zero_from and _bits(part[:, :, c.zero_from:].contiguous()).any():
            fails.append("partials: nonzero where the reference is identically zero")
        acc = torch.zeros_like(part[0])
        for s in range(c.nsplit):
            acc = acc + part[s]
        if not torch.equal(_bits(acc.to(BF16)), _bits(y)):
            fails.append("y is not bf16 of the partials added in split order")
    print(f"\nTABLE fwd {name:<14} y={fy:.2f} part={fp:.3f} sum={fs:.3f} rnd={rnd:.2f}")
    assert not fails, "\n".join(fails)


@gpu
@pytest.mark.parametrize("name", list(FWD))
def test_conv_fwd_deterministic_and_slice_invariant(name):
    """Two runs over differently pre-filled outputs, and the last sample repacked as a B = 1 problem."""
    c, a, b = FWD[name], _run_fwd(name), _run_fwd(name, "three")
    assert b["intact"]
    keys = ("y", "part") if c.nsplit else ("y",)
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{k}: two runs differ"
    if c.B > 1:
        s = _run_fwd(name, "nan", c.B - 1)
        v = c.V // c.B
        assert s["intact"]
        assert torch.equal(_bits(s["y"]), _bits(a["y"][-v:])), "y: the B = 1 repack of a sample differs from its slice"
        if c.nsplit:
            assert torch.equal(_bits(s["part"]), _bits(a["part"][:, -v:].contiguous())), "partials: the same"


def _check_wgrad(name, out):
    """(worst partial, sum) as fractions of the f32 allowance, after the exact checks."""
    c = WGRAD[name]
    ns, part = out["ns"], out["part"]
    R, Lv = _wgrad_rows(c.V, c.S[2], ns)
    assert ns >= c.min_ns, f"lci_conv3_wgrad_splits gave {ns} splits, the case needs {c.min_ns}"
    if c.empty_last:
        assert ns > 1 and (ns - 1) * Lv >= R, f"ns = {ns}, Lv = {Lv}, R = {R}: the last split is not empty here"
    ref = _wg_ref(name, ns)
    fails = []
    if not out["intact"]:
        fails.append("guard band of the partials written")
    if not torch.isfinite(part).all():
        fails.append("partials: non-finite entries left")
    fp = 0.0
    for s in range(ns):
        if not ref[s].any():
            if _bits(part[s]).any():
                fails.append(f"split {s}: nonzero where the reference is identically zero")
        else:
            fp = max(fp, _frac_f32(part[s], ref[s]))
    fs = _frac_f32(part.double().sum(0), ref.sum(0))
    if c.empty_last and ref[ns - 1].any():
        fails.append("the reference of the last split is not zero")
    if not fp <= 1.0:
        fails.append(f"partials: per-element error {fp:.3f} x the allowance")
    if not fs <= 1.0:
        fails.append(f"sum of the partials: per-element error {fs:.3f} x the allowance")
    assert not fails, "\n".join(fails)
    return fp, fs


@gpu
@pytest.mark.parametrize("name", list(WGRAD))
def test_conv_wgrad_vs_fp64(name):
    """Every voxel split's partial and their sum per element against fp64; a second run over a 3.0-pre-filled workspace
    is bitwise equal."""
    out = _run_wgrad(name)
    fp, fs = _check_wgrad(name, out)
    print(f"\nTABLE wgrad {name:<14} ns={out['ns']} part={fp:.3f} sum={fs:.3f}")
    b = _run_wgrad(name, "three")
    assert b["intact"] and torch.equal(_bits(out["part"]), _bits(b["part"])), "two runs differ"


@gpu
@pytest.mark.parametrize("name", [n for n, c in WGRAD.items() if c.v5_too])
def test_conv_wgrad_register_staging_equals_dma(name, monkeypatch):
    """The (1, 3, WC) tiles with LCI_WGRAD_DMA=0 (conv3_wgrad5_kernel<1, 3, WC>): within the fp64 bounds and bitwise
    equal to the default (conv3_wgrad6_kernel<WC>)."""
    v6 = _run_wgrad(name)
    monkeypatch.setenv("LCI_WGRAD_DMA", "0")
    v5 = _run_wgrad(name, "nan", False)
    _check_wgrad(name, v5)
    assert v5["ns"] == v6["ns"] and torch.equal(_bits(v5["part"]), _bits(v6["part"]))


@gpu
@pytest.mark.parametrize("what,nsplit,bad", [
    ("Cout48", 0, dict(Cout=48)), ("KD2", 0, dict(KD=2)), ("KD1_D2", 0, dict(KD=1)), ("x_off8", 0, dict(x_offset=8)),
    ("split_Cin16", 2, dict(Cin=16)), ("split_null_part", 2, dict(null_part=True)), ("nsplit10", 10, dict(nsplit=10)),
    ("Cout48_split", 2, dict(Cout=48)), ("wgrad_Cin16", None, dict(Cin=16))])
def test_conv_host_checks(what, nsplit, bad):
    """Each invalid call raises LciError and leaves the NaN-pre-filled outputs untouched. The problem is 1 x (2, 3, 4),
    32 -> 32, KD = 3 (9 slabs); every buffer is sized for the valid extents, which no invalid value exceeds."""
    g = torch.Generator().manual_seed(77)
    x = _randn_bf16(g, 1, 2, 3, 4, 32)
    if nsplit is None:
        assert _launch_wgrad(x, _randn_bf16(g, 1, 2, 3, 4, 32), 3, float("nan"), bad)
    else:
        assert _launch_fwd(x, _randn_bf16(g, 32, 27, 32, scale=0.03), 3, nsplit, float("nan"), bad)
