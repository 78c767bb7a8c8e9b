"""GPU: every FFT plan of the Hyena long convolution and every short-conv / gate kernel (csrc/hyena.hip) called through
the C entry points on caller-owned buffers, per element against fp64.

Entry points: lci_fft_size, lci_fft_twiddles, lci_fftconv_spectrum, lci_fftconv_fwd, lci_fftconv_bwd,
lci_fftconv_bwd_det; lci_hyena_pre_fwd, lci_hyena_pre_bwd, lci_hyena_pre_bwd_det, lci_hyena_post_fwd,
lci_hyena_post_bwd. Every buffer is a view inside a larger allocation with 64-element guard bands on both sides (256 B
of f32, 128 B of bf16: the views keep their 16-byte alignment). The guards of the inputs (u, dy, k, D, z, w, bias, dvg,
gx2, y, x2, dout) hold NaN; outputs and all scratch (tw, K, SK, S, S2, Su, the deterministic workspaces) are pre-filled,
once with NaN and once with 3.0, and must come back finite, with their guard bands bitwise untouched and bitwise the
same for both fills (no pass reads scratch it did not write; no path here uses float atomics except the dD of the
row_dot_kernel<false> form and the dw / db of the default lci_hyena_pre_bwd, which accumulate into zeroed buffers and
are held to the fp64 bound only). One seeded CPU generator per case.

FFT long conv. Reference, fp64 on the same f32 inputs (the formulas of test_fftconv_c4_length_subset):
  y = irfft(rfft(u, 2L) rfft(k, 2L))[:L] + D u;  du = corr(dy, k) + D dy;  dk = sum_rows corr(dy, u);  dD = sum dy u
and for L <= 512 the direct double sums y[t] = sum_{s<=t} k[t-s] u[s], du[s] = sum_{t>=s} k[t-s] dy[t], dk[j] =
sum_rows sum_t dy[t] u[t-j] (Toeplitz products), which the fp64 FFT must match to 1e-12 and which are then the reference.
Inputs: u, dy ~ N(0, 1), k ~ N(0, 1) / sqrt(L) with no decay (a wrap-around or padding term is as large as any other),
D ~ N(0, 1) distinct per channel.

Plans (restated from fft_plan / launch_col / launch_row; e = ceil(log2(2L)), n = 2^e = n1 n2):
  e 1..8    n2 = 2, n1 = 2^(e-1): fft_col_fwd/inv_kernel (LDS columns, G = 2), fft_row_kernel
  e 9..11   n1 = 256, n2 = 2/4/8: the same LDS column kernels (G = n2: gw = 16 does not divide n2), fft_row_kernel
  e 12, 13  n1 = 256, n2 = 16/32: fft_colw_fwd/inv_kernel<16, 4096, 256, 1>, fft_row_kernel
  e 14..16  n1 = 256, n2 = 64/128/256: fft_colw_*<16, 4096, 256, 4> (GP = 4 prefetch; the forward column pass only when
            L % 4 == 0, else GP = 1), fft_row_kernel
  e 17      n1 = 256, n2 = 512: <16, 4096, 256, 4> + fft_row512_kernel
  e 18      n1 = 512: <8, 4096, 256, 1> + fft_row512_kernel
  (e 19: n1 = 1024, <16, 16384, 512, 4> + row512: test_hyena_gpu.py::test_fftconv_c4_length_subset, not repeated)
Not reachable, hence untested: `thr = a.n2 >= 1024 ? 512 : 256` in launch_row and the `e - ln1 > 10` line of fft_plan
(n2 never exceeds 512: e >= 17 is overridden to n2 = 512).

Cases:
  plan sweep   for every e = 1..18: L = 2^(e-1) (no padding; L % 4 == 0 from e = 3), L = 2^(e-2) + 1 (most padding, odd:
               the scalar row paths, the forward's GP = 1 at e = 14..17; e = 1: L = 1 only) and, from e = 5,
               L = 3 2^(e-3) (not a power of two, L % 4 == 0). R = 3, C = 2 (a half-empty last pair), forward (with Su)
               and the full backward (dk + dD, from that Su).
  batching     L = 4096 (e 13, fft_row_kernel: PB = 4 pairs forward, 2 backward with dk): (R, C) = (1, 2), (2, 2),
               (5, 1), (9, 3), (10, 2): P = 1, 1, 3, 5, 5, i.e. forward batches 4 + 1 and backward 2 + 2 + 1 at P = 5,
               R = 10 with no empty half. L = 32772 (e 17, fft_row512_kernel: nw = the largest divisor of P up to 4):
               (R, C) = (1, 2), (3, 2), (5, 1), (7, 3), (9, 2), (11, 2): P = 1, 2, 3, 4, 5, 6, nw = 1, 2, 3, 4, 1, 3 (every
               width of the cross-wave dk reduction; P = 5 is five pairs serially in one wave). Full backward.
  forms        at e 10 (L = 512), e 15 (L = 16384) and e 17 (L = 32772), R = 3, C = 2: forward with and without Su (y
               bitwise equal); backward from that Su and with Su null (the S2 path: du / dk bitwise equal, so Su holds
               the column spectra a column-only run produces); backward with (dk, dD), (dk), (dD: row_dot_kernel<false>
               on a zeroed dD) and neither; lci_fftconv_bwd_det with (dk, dD) and with (dD); D folded into the spectrum
               (Dv to lci_fftconv_spectrum, null later: what kernels.py does; every other case here) against D applied
               by the column passes (Dv null in the spectrum, given to fwd / bwd), each against fp64.
  impulses     at e 8, 11, 13, 15, 17, 18 (L = 128, 1024, 4096, 16384, 65536, 131072), D = 0: rows u = delta_s for
               s in {0, 1, n2 - 1, n2, L / 2, L - 1} (C = 2): y[t] = k[t - s] for t >= s and y[t] = 0 for t < s (strict
               causality), both within 2e-5 max|k| (the allowance of the non-zero part).
  odd_offset   L = 4097 with u, k, dy, y, du all at a 4-byte offset (the scalar paths need no more), forward + backward.
  offset views kernels.fftconv on u, k taken as 4-byte-offset views of larger tensors at L = 4096 and 16384 (L % 4 == 0:
               kernels.py clones them), forward and backward at the fp64 bounds.
  host checks  L = 0, L = 262145, lci_fftconv_bwd_det with dD, no dk and a null dd_ws, an 8-byte-offset K / S / tw
               and a 4-byte-offset u / y / dy / du at L % 4 == 0 each raise LciError with the NaN outputs untouched.

Gate kernels. Reference: the fp64 torch composite of test_hyena_gpu.py::test_hyena_short_conv_gate_vs_torch (a causal
depthwise conv1d, per head x1 / x2 / v, vg = v x1; gradients by fp64 autograd) on inputs rounded to the I/O dtype
first; post: out = y x2, dy = dout x2, dx2 = dout y. hg_v3_ok sends bf16 with hd % 8 == 0, D % 8 == 0, L % 4 == 0 and
16-byte pointers to the v3 kernels (64-token tiles); everything else runs the v2 register-ring kernels (128-token tiles).
  (BB, L, H, hd, K, dtype)
  v3_k1..8     2, 132, 2, 40, 1..8, bf16, bias at odd K: hyena_pre_fwd3_kernel<K>, hyena_pre_bwd3_kernel<K>; tiles
               64 / 64 / 4, D = 80: a partly filled second channel block, a head seam inside block 0
  v3_pre0      2, 4, 1, 8, 8, bf16: every tap reaches before token 0
  v3_one_tile  1, 64, 2, 32, 5, bf16: exactly one tile
  v3_seam      3, 68, 3, 24, 8, bf16: a halo of 7 across the tile seam, D = 72
  v3_persist   32, 1028, 1, 8, 3, bf16: 17 tiles, gx = 512 / (1 x 32) = 16: workgroup 0 takes two tiles (ntiles > gx
               asserted from the restated rule); default and _det backward
  v2_k1..8     2, 130, 2, 40, 1..8, f32: hyena_pre_fwd2_kernel<float, K>, hyena_pre_bwd2_kernel<float, K>; tiles 128 / 2
  v2_persist_f32 / _bf16   128, 2050, 1, 8, 3: L % 4 = 2 (bf16 falls to v2); 17 tiles, gx = 2048 / 128 = 16 (asserted);
               default and _det backward
  v2_odd_L     2, 131, 2, 40, 5, bf16: L % 4 != 0 -> <bf16, 5>
  v2_hd20      2, 132, 2, 20, 5, bf16: hd % 8 != 0
  v2_z_off8    2, 132, 2, 40, 5, bf16 with z offset by 8 bytes
  post         (BB, L, D) = (2, 4, 8), (1, 64, 64), (2, 132, 80), (3, 68, 72) in bf16 (hyena_post_fwd3 / bwd3_kernel)
               and f32 (hyena_post_fwd / bwd_kernel<float>); bf16 fallbacks to <bf16>: (2, 131, 80), (2, 132, 20) and
               (2, 132, 80) with x2 offset by 8 bytes

Bounds, per element against fp64 on the rounded operands (all from the project's own tests):
  y                      |err| <= 2e-5 max|ref| over that tensor (the forward bound of test_hyena_gpu.py, in max-norm)
  du, dk, dD             1e-4 max|ref|
  f32 vg, dy, x2, dz, out, dx2   1e-5 max|ref|
  dw, db                 1e-4 max|ref|
  bf16 x2, out, dx2, dz  2^-8 |ref| + 1e-4 max|ref| (test_scan_kernel_gpu.py's rule for one bf16 rounding)
The FFT bounds are loose: torch's own f32 FFT of these inputs on the CPU errs by 0.5 - 2.5e-7 max|ref|. So every FFT
case also computes that f32 CPU FFT evaluation of the same formulas and the ratio (kernel's largest error) / (f32 FFT's
largest error) for y, du and dk, the denominator floored at 2^-24 max|ref| (half an ulp of the largest value: where the
CPU happens to be exact, at L = 1, 2, a rounded f32 result still carries that much). Second assertion: every ratio
<= 4 x RATIO_MAX, RATIO_MAX the largest ratio measured over all plans (below); the factor 4 is the headroom for another
CPU's FFT and other inputs.

Measured on an MI355X. Every bitwise check held. FFT: per plan the largest per-element error over the plan's lengths
as a fraction of its allowance (frac) and its ratio to the f32 CPU FFT's largest error (ratio); the impulse rows as
fractions of 2e-5 max|k|. The kernels sit at 0.1 - 1.3 % of the project's bounds and at 0.3 - 2.3 x the error of torch's
f32 FFT; no plan stands out from its neighbours (the largest ratio is 2.31, du at L = 16; RATIO_MAX). The ratios below 1
belong to the lengths whose 2L is not a power of two (odd L, L = 32772), where the CPU's mixed-radix / Bluestein FFT
errs more than at a power of two while the kernels, which always run n = 2^e, do not.
  plan                 y frac ratio  du frac ratio  dk frac ratio  dD frac   lengths
  e  1                 0.0033 0.95   0.0004 0.66    0.0002 0.40    0.0002    1
  e  2                 0.0014 0.47   0.0007 0.46    0.0032 2.17    0.0069    2
  e  3                 0.0036 1.12   0.0009 1.52    0.0008 0.78    0.0006    4, 3
  e  4                 0.0041 1.30   0.0008 1.12    0.0009 1.32    0.0005    8, 5
  e  5                 0.0059 1.56   0.0014 2.31    0.0012 1.01    0.0013    16, 9, 12
  e  6                 0.0093 1.89   0.0014 1.88    0.0016 1.25    0.0010    32, 17, 24
  e  7                 0.0083 1.73   0.0014 1.27    0.0018 0.84    0.0022    64, 33, 48
  e  8                 0.0067 1.08   0.0016 1.19    0.0016 0.85    0.0010    128, 65, 96
  e  9                 0.0065 0.96   0.0012 1.05    0.0022 1.27    0.0018    256, 129, 192
  e 10                 0.0084 1.61   0.0016 1.99    0.0017 1.12    0.0029    512, 257, 384
  e 11                 0.0104 1.22   0.0020 1.10    0.0018 1.00    0.0016    1024, 513, 768
  e 12                 0.0130 1.16   0.0021 1.06    0.0026 1.22    0.0053    2048, 1025, 1536
  e 13                 0.0104 1.91   0.0024 1.74    0.0024 1.16    0.0032    4096, 2049, 3072
  e 14                 0.0107 1.78   0.0029 1.97    0.0029 1.26    0.0052    8192, 4097, 6144
  e 15                 0.0128 1.14   0.0027 1.50    0.0031 1.44    0.0031    16384, 8193, 12288
  e 16                 0.0124 2.00   0.0022 1.70    0.0029 1.23    0.0027    32768, 16385, 24576
  e 17                 0.0131 1.37   0.0027 1.55    0.0029 1.26    0.0018    65536, 32769, 49152
  e 18                 0.0123 1.50   0.0025 1.48    0.0028 1.14    0.0037    131072, 65537, 98304
  L 4096  R 1  C 2     0.0092 2.18   0.0019 2.12    0.0018 0.77    0.0006
  L 4096  R 2  C 2     0.0132 1.38   0.0023 1.27    0.0026 1.39    0.0017
  L 4096  R 5  C 1     0.0101 1.92   0.0019 2.19    0.0026 1.25    0.0005
  L 4096  R 9  C 3     0.0120 1.22   0.0026 1.15    0.0025 1.41    0.0020
  L 4096  R 10 C 2     0.0107 1.79   0.0020 1.61    0.0028 1.09    0.0038
  L 32772 R 1  C 2     0.0120 0.38   0.0020 0.29    0.0026 0.32    0.0013
  L 32772 R 3  C 2     0.0107 0.98   0.0024 1.07    0.0029 0.32    0.0032
  L 32772 R 5  C 1     0.0116 0.62   0.0025 0.63    0.0026 0.33    0.0012
  L 32772 R 7  C 3     0.0128 0.53   0.0022 0.43    0.0023 0.34    0.0021
  L 32772 R 9  C 2     0.0111 0.77   0.0024 1.00    0.0027 0.37    0.0020
  L 32772 R 11 C 2     0.0116 0.61   0.0023 0.70    0.0025 0.30    0.0022
  impulses             L 128: 0.005 (t >= s) / 0.005 (t < s); 1024: 0.006 / 0.006; 4096: 0.014 / 0.007; 16384: 0.011 /
                       0.007; 65536: 0.015 / 0.008; 131072: 0.014 / 0.009
Gate kernels, fractions of the allowance: the bf16 outputs (x2, dz, out, dx2) sit at 0.70 - 0.95, i.e. at the one bf16
rounding the bound allows (v3 and v2 alike: v3_k1..8 x2 0.88 - 0.93, dz 0.87 - 0.93; v3_persist 0.94 / 0.91;
v2_persist_bf16 0.95 / 0.92; the three fallbacks 0.92 / 0.88; post out 0.70 - 0.95, dx2 0.81 - 0.90); the f32 outputs at
0.002 - 0.016 of theirs (vg 0.005 - 0.016, f32 x2 / dz 0.003 - 0.015, post f32 0.002 - 0.005, the bf16 post's f32 dy exact);
dw / db at 0.001 - 0.002, and 0.006 - 0.013 for the atomic sums of the three persistent cases against 0.001 - 0.003 from
lci_hyena_pre_bwd_det.
"""
import dataclasses
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64            # guard-band elements on either side (256 B of f32, 128 B of bf16: keeps the 16-byte alignment)
SENTINEL = -7.0       # exact in bf16 and f32
U_BF16 = 2.0 ** -8
FILLS = {"nan": float("nan"), "three": 3.0}
HG_TT, HY_TT = 64, 128            # csrc/hyena.hip: tokens per tile of the v3 and the v2 gate kernels
RATIO_MAX = 2.31                  # largest (kernel error) / (f32 CPU FFT error) measured over all plans (docstring)


# ------------------------------------------------------------------------------------------------ buffers
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


class _In:
    """A CPU tensor on the device as a contiguous view inside a flat buffer whose guard bands hold NaN. `shift` moves
    the view by that many elements into the trailing guard (a pointer that is not 16-byte aligned)."""

    def __init__(self, t, dtype=F32, shift=0):
        n = t.numel()
        self.flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.view = self.flat[GUARD + shift:GUARD + shift + n].view(t.shape)
        self.view.copy_(t)

    def ptr(self):
        return self.view.data_ptr()


class _Out:
    """An output or scratch buffer of `shape` inside a flat buffer: sentinel guard bands, the view pre-filled by `fill`."""

    def __init__(self, shape, fill, dtype=F32, shift=0):
        n = math.prod(shape)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.flat[self.lo:self.hi].view(shape)
        self.view.fill_(fill)
        self.before = self.flat.clone()

    def guards_intact(self):
        a, b = _bits(self.flat), _bits(self.before)
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.hi:], b[self.hi:])

    def unchanged(self):
        return torch.equal(_bits(self.flat), _bits(self.before))

    def ptr(self):
        return self.view.data_ptr()

    def cpu(self):
        return self.view.cpu()


def _ptr(b):
    return None if b is None else b.ptr()


def _lib():
    from long_context_biomedical_imaging_amd import _lib as lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ metrics
def _maxerr(x, ref):
    """Largest |x - ref|; a NaN gives inf."""
    err = (x.double() - ref).abs()
    return torch.where(torch.isnan(err), torch.full_like(err, math.inf), err).max().item()


def _frac(x, ref, tol):
    """Largest |err| / (tol max|ref|)."""
    return _maxerr(x, ref) / (tol * ref.abs().max().item())


def _frac_bf16(x, ref):
    """Largest |err| / (2^-8 |ref| + 1e-4 max|ref|)."""
    err = (x.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    return (err / (U_BF16 * ref.abs() + 1e-4 * ref.abs().max())).max().item()


def _frac_io(x, ref, dtype):
    return _frac_bf16(x, ref) if dtype == BF16 else _frac(x, ref, 1e-5)


# ------------------------------------------------------------------------------------------------ FFT: fp64 side
def _plan(L):
    """(e, n1, n2) of fft_plan, restated."""
    e = 1
    while (1 << e) < 2 * L:
        e += 1
    ln1 = min(e, 8)
    if e - ln1 == 0:
        ln1 = e - 1
    if 17 <= e <= 19:
        ln1 = e - 9
    return e, 1 << ln1, 1 << (e - ln1)


def _conv_formulas(u, k, D, dy):
    """The four formulas of the module docstring in u's dtype, through torch.fft at n = 2L."""
    L = u.shape[-1]
    n = 2 * L
    rf, irf = torch.fft.rfft, torch.fft.irfft
    kf = rf(k, n)
    y = irf(rf(u, n) * kf, n)[..., :L] + u * D[:, None]
    du = irf(rf(dy.flip(-1), n) * kf, n)[..., :L].flip(-1) + dy * D[:, None]
    dk = irf(rf(dy.flip(-1), n) * rf(u, n), n)[..., :L].flip(-1).sum(0)
    return dict(y=y, du=du, dk=dk, dD=(dy * u).sum((0, 2)))


def _direct(u, k, D, dy):
    """The same by direct fp64 sums (L <= 512): T[c, t, s] = k[c, t - s] for s <= t."""
    L = u.shape[-1]
    t = torch.arange(L)
    lag = t[:, None] - t[None, :]
    T = torch.where(lag >= 0, k[:, lag.clamp_min(0)], torch.zeros((), dtype=F64))          # (C, t, s)
    y = torch.einsum("cts,rcs->rct", T, u) + u * D[:, None]
    du = torch.einsum("cts,rct->rcs", T, dy) + dy * D[:, None]
    U = torch.where(lag >= 0, u[..., lag.clamp_min(0)], torch.zeros((), dtype=F64))        # (R, C, t, j) = u[t - j]
    dk = torch.einsum("rct,rctj->cj", dy, U)
    return dict(y=y, du=du, dk=dk, dD=(dy * u).sum((0, 2)))


@functools.lru_cache(maxsize=4)
def _fft_case(R, C, L, seed, zero_D=False):
    """(inputs, fp64 reference, largest error of the f32 CPU FFT per output); computed once, never modified."""
    g = torch.Generator().manual_seed(seed)
    u, dy = torch.randn(R, C, L, generator=g), torch.randn(R, C, L, generator=g)
    k = torch.randn(C, L, generator=g) / math.sqrt(L)
    D = torch.randn(C, generator=g) * (0.0 if zero_D else 1.0)
    inp = dict(u=u, k=k, D=D, dy=dy)
    ref = _conv_formulas(u.double(), k.double(), D.double(), dy.double())
    if L <= 512:
        direct = _direct(u.double(), k.double(), D.double(), dy.double())
        for key, r in direct.items():
            assert _maxerr(ref[key], r) <= 1e-12 * r.abs().max().item(), f"fp64 FFT and direct sums differ in {key}"
        ref = direct
    f32 = _conv_formulas(u, k, D, dy)
    e32 = {key: _maxerr(f32[key], ref[key]) for key in ref}
    return inp, ref, e32


# ------------------------------------------------------------------------------------------------ FFT: device side
def _fft_run(inp, fill, *, fold=True, su=True, bwd="kd", det=False, shift=0, fwd=True, bwd_su=None):
    """spectrum -> forward -> backward on fresh guarded buffers. fold: D to lci_fftconv_spectrum (else to fwd / bwd);
    su: the forward keeps Su; bwd_su (default su): the backward takes it (else S2); bwd: which of dk ("k") and dD ("d")
    the backward computes, None: no backward; det: lci_fftconv_bwd_det. Returns the outputs on the CPU and `intact`."""
    lib = _lib()
    fill = FILLS[fill]
    u, k, D, dy = inp["u"], inp["k"], inp["D"], inp["dy"]
    R, C, L = u.shape
    n, P, s = int(lib.load().lci_fft_size(L)), (R + 1) // 2, _stream()
    assert n == 1 << _plan(L)[0]
    ud, kd, Dd, dyd = _In(u, shift=shift), _In(k, shift=shift), _In(D), _In(dy, shift=shift)
    outs = {}

    def out(name, shape, f=fill, sh=0):
        outs[name] = _Out(shape, f, shift=sh)
        return outs[name]

    tw, K, SK = out("tw", (n, 2)), out("K", (C, n, 2)), out("SK", (C, n, 2))
    lib.call("lci_fft_twiddles", tw.ptr(), n, s)
    lib.call("lci_fftconv_spectrum", kd.ptr(), Dd.ptr() if fold else None, K.ptr(), SK.ptr(), tw.ptr(), C, L, s)
    Dv = None if fold else Dd.ptr()
    res, Su = {}, None
    if fwd:
        y, S = out("y", (R, C, L), sh=shift), out("S", (C * P, n, 2))
        Su = out("Su", (C * P, n, 2)) if su else None
        lib.call("lci_fftconv_fwd", ud.ptr(), K.ptr(), Dv, y.ptr(), S.ptr(), _ptr(Su), tw.ptr(), R, C, L, s)
    if bwd is not None:
        want_k, want_d = "k" in bwd, "d" in bwd
        use_su = (su if bwd_su is None else bwd_su) and want_k
        du, Sb = out("du", (R, C, L), sh=shift), out("Sb", (C * P, n, 2))
        dk = out("dk", (C, L), sh=shift) if want_k else None
        dD = out("dD", (C,), fill if det else 0.0) if want_d else None
        S2 = out("S2", (C * P, n, 2)) if want_k and not use_su else None
        SKb = out("SKb", (C, n, 2)) if want_k else None
        args = (dyd.ptr(), ud.ptr(), K.ptr(), Dv, du.ptr(), _ptr(dk), _ptr(dD), Sb.ptr(), _ptr(S2),
                Su.ptr() if use_su else None, _ptr(SKb), tw.ptr())
        if det:
            nb = int(lib.load().lci_fftconv_bwd_det_ws_bytes(R, C, L))
            ws = out("ws", (nb // 4,)) if want_d and not want_k else None
            lib.call("lci_fftconv_bwd_det", *args, _ptr(ws), R, C, L, s)
        else:
            lib.call("lci_fftconv_bwd", *args, R, C, L, s)
    torch.cuda.synchronize()
    for name in ("y", "du", "dk", "dD"):
        if name in outs:
            res[name] = outs[name].cpu()
    res["intact"] = all(o.guards_intact() for o in outs.values())
    return res


def _check_fft(res, ref, e32, keys, tag, fails, table=None):
    """Each output in `keys` finite and within its fp64 bound; the ratio to the f32 CPU FFT's error for y, du, dk."""
    if not res["intact"]:
        fails.append(f"{tag}: a guard band was written")
    for key in keys:
        x, r = res[key], ref[key]
        if not torch.isfinite(x).all():
            fails.append(f"{tag} {key}: non-finite entries left")
        fr = _frac(x, r, 2e-5 if key == "y" else 1e-4)
        if not fr <= 1.0:
            fails.append(f"{tag} {key}: per-element error {fr:.3g} x the allowance")
        ratio = float("nan")
        if key != "dD":
            ratio = _maxerr(x, r) / max(e32[key], 2.0 ** -24 * r.abs().max().item())
            if RATIO_MAX is not None and not ratio <= 4 * RATIO_MAX:
                fails.append(f"{tag} {key}: error {ratio:.3g} x the f32 CPU FFT's, over 4 x {RATIO_MAX}")
        if table is not None:
            table.append(f"{key}={fr:.4f}/{ratio:.2f}")


def _same(a, b, keys, tag, fails):
    for key in keys:
        if not torch.equal(_bits(a[key]), _bits(b[key])):
            fails.append(f"{tag}: {key} differs bit for bit")


def _full_case(R, C, L, seed, label):
    """Forward (with Su) and full backward, twice over differently pre-filled buffers."""
    inp, ref, e32 = _fft_case(R, C, L, seed)
    fails, table = [], []
    a = _fft_run(inp, "nan")
    b = _fft_run(inp, "three")
    _check_fft(a, ref, e32, ("y", "du", "dk", "dD"), "nan", fails, table)
    if not b["intact"]:
        fails.append("three: a guard band was written")
    _same(a, b, ("y", "du", "dk", "dD"), "NaN- and 3.0-filled runs", fails)
    e, n1, n2 = _plan(L)
    print(f"\nTABLE fft {label:<14} e={e:<2} n1={n1:<4} n2={n2:<3} R={R} C={C} L={L}: frac/ratio " + " ".join(table))
    assert not fails, "\n".join(fails)


def _sweep_lengths():
    out = []
    for e in range(1, 19):
        Ls = [1] if e == 1 else [1 << (e - 1), (1 << (e - 2)) + 1]
        if e >= 5:
            Ls.append(3 << (e - 3))
        out += [(e, L) for L in dict.fromkeys(Ls)]   # (e = 2: both are L = 2)
    return out


@pytest.mark.parametrize("e,L", _sweep_lengths(), ids=lambda v: str(v))
def test_fftconv_plan_sweep(e, L):
    """Every plan e = 1..18 at three lengths, R = 3, C = 2: forward and full backward per element against fp64."""
    assert _plan(L)[0] == e
    _full_case(3, 2, L, 1000 + L, f"sweep_{L}")


@pytest.mark.parametrize("L,R,C", [(4096, 1, 2), (4096, 2, 2), (4096, 5, 1), (4096, 9, 3), (4096, 10, 2),
                                   (32772, 1, 2), (32772, 3, 2), (32772, 5, 1), (32772, 7, 3), (32772, 9, 2),
                                   (32772, 11, 2)])
def test_fftconv_pair_batching(L, R, C):
    """Row-pass batching: fft_row_kernel's 4 + 1 / 2 + 2 + 1 batches and every fft_row512_kernel wave count."""
    _full_case(R, C, L, 2000 + 16 * R + C, f"batch_{L}_{R}x{C}")


@pytest.mark.parametrize("L", [512, 16384, 32772])
def test_fftconv_entry_point_forms(L):
    """Su kept or not, every (dk, dD) form of both backward entry points, D folded or applied by the column passes."""
    inp, ref, e32 = _fft_case(3, 2, L, 3000 + L)
    fails = []
    runs = {}
    for name, kw in {"su": dict(su=True), "nosu": dict(su=False),
                     "su_fwd_s2_bwd": dict(su=True, bwd_su=False),
                     "k": dict(bwd="k"), "d": dict(bwd="d", fwd=False), "none": dict(bwd="", fwd=False),
                     "det_kd": dict(det=True), "det_d": dict(det=True, bwd="d", fwd=False),
                     "unfolded": dict(fold=False), "unfolded_d": dict(fold=False, bwd="d", fwd=False)}.items():
        keys = tuple(x for x in ("y", "du", "dk", "dD")
                     if (x == "y" and kw.get("fwd", True)) or x == "du"
                     or (x == "dk" and "k" in kw.get("bwd", "kd")) or (x == "dD" and "d" in kw.get("bwd", "kd")))
        for fill in FILLS:
            runs[name, fill] = _fft_run(inp, fill, **kw)
            _check_fft(runs[name, fill], ref, e32, keys, f"{name}/{fill}", fails)
        # the dD of row_dot_kernel<false> is a sum of float atomics: held to the fp64 bound only
        exact = tuple(x for x in keys if not (name in ("d", "unfolded_d") and x == "dD"))
        _same(runs[name, "nan"], runs[name, "three"], exact, f"{name}: NaN- and 3.0-filled runs", fails)
    _same(runs["su", "nan"], runs["nosu", "nan"], ("y",), "forward with and without Su", fails)
    _same(runs["su", "nan"], runs["nosu", "nan"], ("du", "dk", "dD"), "backward from the kept Su and from S2", fails)
    _same(runs["su", "nan"], runs["su_fwd_s2_bwd", "nan"], ("y", "du", "dk", "dD"), "Su kept but S2 used", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("L", [128, 1024, 4096, 16384, 65536, 131072])
def test_fftconv_unit_impulses(L):
    """u = delta_s, D = 0: y[t] = k[t - s] for t >= s and strictly zero influence before s, for s at the column-group
    and length edges, within 2e-5 max|k|."""
    e, n1, n2 = _plan(L)
    ss = [0, 1, n2 - 1, n2, L // 2, L - 1]
    C = 2
    g = torch.Generator().manual_seed(4000 + L)
    k = torch.randn(C, L, generator=g) / math.sqrt(L)
    u = torch.zeros(len(ss), C, L)
    want = torch.zeros(len(ss), C, L, dtype=F64)
    for r, s in enumerate(ss):
        u[r, :, s] = 1.0
        want[r, :, s:] = k[:, :L - s].double()
    inp = dict(u=u, k=k, D=torch.zeros(C), dy=u)
    a = _fft_run(inp, "nan", bwd=None)
    b = _fft_run(inp, "three", bwd=None)
    allow = 2e-5 * k.abs().max().item()
    err = (a["y"].double() - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    fails = []
    for r, s in enumerate(ss):
        after, before = err[r, :, s:].max().item(), (err[r, :, :s].max().item() if s else 0.0)
        print(f"\nTABLE impulse L={L} s={s}: t>=s {after / allow:.4f} t<s {before / allow:.4f} of the allowance")
        if not after <= allow:
            fails.append(f"s = {s}: y[t >= s] off k[t - s] by {after / allow:.3g} x the allowance")
        if not before <= allow:
            fails.append(f"s = {s}: y[t < s] is {before / allow:.3g} x the allowance (causality)")
    if not (a["intact"] and b["intact"]):
        fails.append("a guard band was written")
    _same(a, b, ("y",), "NaN- and 3.0-filled runs", fails)
    assert not fails, "\n".join(fails)


def test_fftconv_odd_length_at_4_byte_offset():
    """L = 4097 (scalar row accesses) with every row tensor at a 4-byte offset: accepted, and within the bounds."""
    inp, ref, e32 = _fft_case(3, 2, 4097, 5000)
    fails = []
    a, b = _fft_run(inp, "nan", shift=1), _fft_run(inp, "three", shift=1)
    _check_fft(a, ref, e32, ("y", "du", "dk", "dD"), "nan", fails)
    _same(a, b, ("y", "du", "dk", "dD"), "NaN- and 3.0-filled runs", fails)
    assert b["intact"] and not fails, "\n".join(fails)


@pytest.mark.parametrize("L", [4096, 16384])
def test_fftconv_module_path_on_offset_views(L):
    """kernels.fftconv on contiguous f32 views at a 4-byte storage offset (L % 4 == 0: copied before the call)."""
    from long_context_biomedical_imaging_amd import kernels
    R, C = 3, 2
    inp, ref, _ = _fft_case(R, C, L, 6000 + L)

    def offset_view(t):
        base = torch.empty(t.numel() + 8, device="cuda")
        v = base[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v.requires_grad_(True)

    u, k, dy = offset_view(inp["u"]), offset_view(inp["k"]), offset_view(inp["dy"]).detach()
    D = inp["D"].cuda().requires_grad_(True)
    y = kernels.fftconv(u, k, D)
    y.backward(dy)
    got = dict(y=y.detach().cpu(), du=u.grad.cpu(), dk=k.grad.cpu(), dD=D.grad.cpu())
    for key, tol in (("y", 2e-5), ("du", 1e-4), ("dk", 1e-4), ("dD", 1e-4)):
        assert _frac(got[key], ref[key], tol) <= 1.0, key


@pytest.mark.parametrize("what", ["L0", "L262145", "det_null_ws", "K_off8", "S_off8", "tw_off8", "Su_off8", "SK_off8",
                                  "u_off4", "y_off4", "dy_off4", "du_off4", "k_off4"])
def test_fftconv_host_checks(what):
    """Each invalid call raises LciError and leaves the NaN-pre-filled outputs and scratch untouched. R = 3, C = 2,
    L = 8 (n = 16); every buffer is sized for the valid call."""
    lib = _lib()
    R, C, L, n, P, s = 3, 2, 8, 16, 2, _stream()
    g = torch.Generator().manual_seed(7)
    nan = float("nan")
    u, dy, k = (_In(torch.randn(*sh, generator=g)) for sh in ((R, C, L), (R, C, L), (C, L)))
    tw, K, SK, S, S2, Su = (_Out(sh, nan) for sh in ((n, 2), (C, n, 2), (C, n, 2), (C * P, n, 2), (C * P, n, 2),
                                                     (C * P, n, 2)))
    y, du, dk, dD, ws = (_Out(sh, nan) for sh in ((R, C, L), (R, C, L), (C, L), (C,), (R * C,)))
    bufs = (tw, K, SK, S, S2, Su, y, du, dk, dD, ws)
    off = lambda b, name, nbytes: b.ptr() + (nbytes if what == f"{name}_off{nbytes}" else 0)  # noqa: E731
    Lbad = {"L0": 0, "L262145": 262145}.get(what, L)
    calls = []
    if what in ("L0", "L262145", "K_off8", "SK_off8", "tw_off8", "k_off4"):
        calls.append(("lci_fftconv_spectrum", off(k, "k", 4), None, off(K, "K", 8), off(SK, "SK", 8), off(tw, "tw", 8),
                      C, Lbad, s))
    if what in ("L0", "L262145", "K_off8", "S_off8", "tw_off8", "Su_off8", "u_off4", "y_off4"):
        calls.append(("lci_fftconv_fwd", off(u, "u", 4), off(K, "K", 8), None, off(y, "y", 4), off(S, "S", 8),
                      off(Su, "Su", 8), off(tw, "tw", 8), R, C, Lbad, s))
    if what != "y_off4" and what != "k_off4":
        bwd = (off(dy, "dy", 4), off(u, "u", 4), off(K, "K", 8), None, off(du, "du", 4), dk.ptr(), dD.ptr(),
               off(S, "S", 8), S2.ptr(), off(Su, "Su", 8), off(SK, "SK", 8), off(tw, "tw", 8))
        if what == "det_null_ws":
            calls.append(("lci_fftconv_bwd_det", *bwd[:5], None, *bwd[6:], None, R, C, L, s))
        else:
            calls.append(("lci_fftconv_bwd", *bwd, R, C, Lbad, s))
            calls.append(("lci_fftconv_bwd_det", *bwd, ws.ptr(), R, C, Lbad, s))
    assert calls
    for c in calls:
        with pytest.raises(lib.LciError):
            lib.call(*c)
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in bufs)


# ------------------------------------------------------------------------------------------------ gate kernels
@dataclasses.dataclass(frozen=True)
class Pre:
    BB: int
    L: int
    H: int
    hd: int
    K: int
    dtype: torch.dtype
    bias: bool = False
    z_shift: int = 0           # elements the z pointer is moved off its 16-byte alignment
    v3: bool = False           # the kernels hg_v3_ok must choose
    persistent: bool = False   # ntiles > gx: a workgroup of the backward takes a second tile; also runs _det

    @property
    def D(self):
        return self.H * self.hd


PRE = {}
for _K in range(1, 9):
    PRE[f"v3_k{_K}"] = Pre(2, 132, 2, 40, _K, BF16, bias=_K % 2 == 1, v3=True)
PRE["v3_pre0"] = Pre(2, 4, 1, 8, 8, BF16, v3=True)
PRE["v3_one_tile"] = Pre(1, 64, 2, 32, 5, BF16, v3=True)
PRE["v3_seam"] = Pre(3, 68, 3, 24, 8, BF16, v3=True)
PRE["v3_persist"] = Pre(32, 1028, 1, 8, 3, BF16, v3=True, persistent=True)
for _K in range(1, 9):
    PRE[f"v2_k{_K}"] = Pre(2, 130, 2, 40, _K, F32)
PRE["v2_persist_f32"] = Pre(128, 2050, 1, 8, 3, F32, persistent=True)
PRE["v2_persist_bf16"] = Pre(128, 2050, 1, 8, 3, BF16, persistent=True)
PRE["v2_odd_L"] = Pre(2, 131, 2, 40, 5, BF16)
PRE["v2_hd20"] = Pre(2, 132, 2, 20, 5, BF16)
PRE["v2_z_off8"] = Pre(2, 132, 2, 40, 5, BF16, z_shift=4)


def _pre_grid(c):
    """(v3, ntiles, gx) of hyena_pre_bwd_launch, restated: hg_v3_ok, then gx = max(1, min(ntiles, budget / (ncy BB)))
    with 64-token tiles and a budget of 512 workgroups (v3) or 128-token tiles and 2048 (v2)."""
    v3 = c.dtype == BF16 and c.hd % 8 == 0 and c.D % 8 == 0 and c.L % 4 == 0 and c.z_shift == 0
    tt, budget = (HG_TT, 512) if v3 else (HY_TT, 2048)
    ntiles, ncy = -(-c.L // tt), -(-c.D // 64)
    return v3, ntiles, max(1, min(ntiles, budget // max(1, ncy * c.BB)))


def _round(t, dtype):
    return t.to(dtype).float()


@functools.lru_cache(maxsize=4)
def _pre_case(name):
    """(inputs holding values of the I/O dtype, fp64 reference); computed once, never modified."""
    c = PRE[name]
    g = torch.Generator().manual_seed(7000 + list(PRE).index(name))
    D = c.D
    inp = dict(z=_round(torch.randn(c.BB, c.L, 3 * D, generator=g), c.dtype),
               w=torch.randn(3 * D, c.K, generator=g) * 0.5,
               b=torch.randn(3 * D, generator=g) * 0.1 if c.bias else None,
               dvg=torch.randn(c.BB, D, c.L, generator=g),
               gx2=_round(torch.randn(c.BB, c.L, D, generator=g), c.dtype))
    zr, wr = inp["z"].double().requires_grad_(True), inp["w"].double().requires_grad_(True)
    br = inp["b"].double().requires_grad_(True) if c.bias else None
    conv = torch.nn.functional.conv1d(zr.transpose(1, 2), wr[:, None], br, padding=c.K - 1, groups=3 * D)[..., :c.L]
    conv = conv.view(c.BB, c.H, 3, c.hd, c.L)
    x1, x2, v = (conv[:, :, i].reshape(c.BB, D, c.L) for i in range(3))
    vg, x2 = v * x1, x2.transpose(1, 2)
    ((vg * inp["dvg"].double()).sum() + (x2 * inp["gx2"].double()).sum()).backward()
    ref = dict(vg=vg.detach(), x2=x2.detach().contiguous(), dz=zr.grad, dw=wr.grad, db=br.grad if c.bias else None)
    return inp, ref


def _pre_run(name, fill, det=False):
    lib = _lib()
    c, (inp, _) = PRE[name], _pre_case(name)
    fill = FILLS[fill]
    D, s, dt = c.D, _stream(), lib.DTYPE[c.dtype]
    z, w = _In(inp["z"], c.dtype, shift=c.z_shift), _In(inp["w"])
    b = _In(inp["b"]) if c.bias else None
    dvg, gx2 = _In(inp["dvg"]), _In(inp["gx2"], c.dtype)
    outs = dict(vg=_Out((c.BB, D, c.L), fill), x2=_Out((c.BB, c.L, D), fill, c.dtype),
                dz=_Out((c.BB, c.L, 3 * D), fill, c.dtype), dw=_Out((3 * D, c.K), fill if det else 0.0))
    if c.bias:
        outs["db"] = _Out((3 * D,), fill if det else 0.0)
    dims = (c.BB, c.L, c.H, c.hd, c.K, s)
    lib.call("lci_hyena_pre_fwd", dt, z.ptr(), w.ptr(), _ptr(b), outs["vg"].ptr(), outs["x2"].ptr(), *dims)
    head = (dt, z.ptr(), w.ptr(), _ptr(b), dvg.ptr(), gx2.ptr(), outs["dz"].ptr(), outs["dw"].ptr(),
            _ptr(outs.get("db")))
    if det:
        nb = int(lib.load().lci_hyena_pre_bwd_det_ws_bytes(c.BB, c.L, c.H, c.hd, c.K))
        assert nb > 0 and nb % (3 * D * (c.K + 1) * 4) == 0
        outs["ws"] = _Out((nb // 4,), fill)
        lib.call("lci_hyena_pre_bwd_det", *head, outs["ws"].ptr(), *dims)
    else:
        lib.call("lci_hyena_pre_bwd", *head, *dims)
    torch.cuda.synchronize()
    res = {k: o.cpu() for k, o in outs.items() if k != "ws"}
    res["intact"] = all(o.guards_intact() for o in outs.values())
    return res


def _check_pre(name, res, tag, fails, table=None):
    c, (_, ref) = PRE[name], _pre_case(name)
    if not res["intact"]:
        fails.append(f"{tag}: a guard band was written")
    for key in ("vg", "x2", "dz", "dw", "db"):
        if ref[key] is None:
            continue
        x = res[key]
        if not torch.isfinite(x.float()).all():
            fails.append(f"{tag} {key}: non-finite entries left")
        if key in ("dw", "db"):
            fr = _frac(x, ref[key], 1e-4)
        elif key == "vg":
            fr = _frac(x, ref[key], 1e-5)
        else:
            fr = _frac_io(x, ref[key], c.dtype)
        if not fr <= 1.0:
            fails.append(f"{tag} {key}: per-element error {fr:.3g} x the allowance")
        if table is not None:
            table.append(f"{key}={fr:.3f}")


@pytest.mark.parametrize("name", list(PRE))
def test_hyena_pre_vs_fp64(name):
    """lci_hyena_pre_fwd and lci_hyena_pre_bwd (and _det on the persistent cases) per element against the fp64
    composite; every written output bitwise the same over NaN- and 3.0-filled buffers."""
    c = PRE[name]
    v3, ntiles, gx = _pre_grid(c)
    assert v3 == c.v3, "the case does not reach the kernels it names"
    if c.persistent:
        assert ntiles > gx, f"ntiles = {ntiles}, gx = {gx}: no workgroup takes a second tile"
    fails, table = [], []
    a, b = _pre_run(name, "nan"), _pre_run(name, "three")
    _check_pre(name, a, "nan", fails, table)
    _check_pre(name, b, "three", fails)
    _same(a, b, ("vg", "x2", "dz"), "NaN- and 3.0-filled runs", fails)
    if c.persistent:
        da, db = _pre_run(name, "nan", det=True), _pre_run(name, "three", det=True)
        _check_pre(name, da, "det/nan", fails, table)
        _same(da, db, ("vg", "x2", "dz", "dw") + (("db",) if c.bias else ()), "_det: NaN- and 3.0-filled runs", fails)
        if not db["intact"]:
            fails.append("det/three: a guard band was written")
    print(f"\nTABLE pre {name:<16} {'v3' if v3 else 'v2'} ntiles={ntiles} gx={gx}: " + " ".join(table))
    assert not fails, "\n".join(fails)


POST = {}
for _dt, _tag in ((BF16, "bf16"), (F32, "f32")):
    for _shape in ((2, 4, 8), (1, 64, 64), (2, 132, 80), (3, 68, 72)):
        POST[f"{_tag}_{_shape[0]}_{_shape[1]}_{_shape[2]}"] = (*_shape, _dt, 0)
POST["bf16_odd_L"] = (2, 131, 80, BF16, 0)
POST["bf16_D20"] = (2, 132, 20, BF16, 0)
POST["bf16_x2_off8"] = (2, 132, 80, BF16, 4)


@pytest.mark.parametrize("name", list(POST))
def test_hyena_post_vs_fp64(name):
    """lci_hyena_post_fwd / _bwd: out = y x2, dy = dout x2, dx2 = dout y per element against fp64 products of the
    rounded operands, bitwise the same over NaN- and 3.0-filled outputs."""
    lib = _lib()
    BB, L, D, dtype, x2_shift = POST[name]
    g = torch.Generator().manual_seed(8000 + list(POST).index(name))
    y = torch.randn(BB, D, L, generator=g)
    x2, dout = (_round(torch.randn(BB, L, D, generator=g), dtype) for _ in range(2))
    yt = y.double().transpose(1, 2)
    ref = dict(out=yt * x2.double(), dy=(dout.double() * x2.double()).transpose(1, 2), dx2=dout.double() * yt)
    runs, fails, table = {}, [], []
    for fill in FILLS:
        yd, x2d, doutd = _In(y), _In(x2, dtype, shift=x2_shift), _In(dout, dtype)
        outs = dict(out=_Out((BB, L, D), FILLS[fill], dtype), dy=_Out((BB, D, L), FILLS[fill]),
                    dx2=_Out((BB, L, D), FILLS[fill], dtype))
        dt, s = lib.DTYPE[dtype], _stream()
        lib.call("lci_hyena_post_fwd", dt, yd.ptr(), x2d.ptr(), outs["out"].ptr(), BB, L, D, s)
        lib.call("lci_hyena_post_bwd", dt, yd.ptr(), x2d.ptr(), doutd.ptr(), outs["dy"].ptr(), outs["dx2"].ptr(), BB,
                 L, D, s)
        torch.cuda.synchronize()
        runs[fill] = {k: o.cpu() for k, o in outs.items()}
        if not all(o.guards_intact() for o in outs.values()):
            fails.append(f"{fill}: a guard band was written")
    for key in ("out", "dy", "dx2"):
        x = runs["nan"][key]
        if not torch.isfinite(x.float()).all():
            fails.append(f"{key}: non-finite entries left")
        fr = _frac(x, ref[key], 1e-5) if key == "dy" else _frac_io(x, ref[key], dtype)
        table.append(f"{key}={fr:.3f}")
        if not fr <= 1.0:
            fails.append(f"{key}: per-element error {fr:.3g} x the allowance")
    _same(runs["nan"], runs["three"], ("out", "dy", "dx2"), "NaN- and 3.0-filled runs", fails)
    print(f"\nTABLE post {name:<16} " + " ".join(table))
    assert not fails, "\n".join(fails)
