"""GPU: every kernel of csrc/norm.hip (instance norm + LeakyReLU, the fused residual tail, training BatchNorm + ReLU)
called through the C entry points on caller-owned buffers, stage by stage, against plain fp64 expressions written here.

Conventions (those of tests/test_conv_kernel_gpu.py): one seeded CPU generator per case; inputs rounded to bf16 before
either side sees them; every buffer a view inside a larger allocation with 64-element guard bands; input guards hold
NaN; outputs are pre-filled with NaN, must come out finite everywhere and leave their guard bands bitwise untouched.
A later stage reads the buffer the earlier stage's kernel wrote, and is judged against fp64 of that buffer, so every
stage is judged apart from the others; the end-to-end checks are separate.

Inputs: x[b, v, c] = bf16(sigma_c randn + mu_c), sigma_c a permutation of linspace(0.25, 3, C), mu_c = sigma_c times
a permutation of linspace(-4, 4, C). Where C >= 16 channel C / 2 is constant at 1.5: every f32 sum of it is exact, its
mean is 1.5 and its variance 0 exactly, so z (and n inside the backward) must be exactly 0 there. Cotangents
dz = bf16(randn + 0.5 + 0.25 nhat), nhat the fp64 normalised input, so mean_V(dn) ~ 0.5 and mean_V(dn n) ~ 0.25: the
backward coefficients are O(1). LeakyReLU / ReLU masks of the fp64 references come from the f32 restatement of the
pre-activation (torch, CPU, from the stats the kernel wrote), which stage 3 / 6 show bitwise equal to the kernel's own.

Instance-norm cases (B, V, C); the regime of each is asserted from a restatement of G = C / 8, rows = 256 / G,
lci_inorm_chunks and chunk = ceil(V / nchunk) (REGIME below), on the device's lci_inorm_chunks:
  rows21    2 x 990 x 96      rows = 21, 4 idle threads, 4 chunks of 248: 11 or 12 voxels per lane
  chunks7   1 x 1551 x 64     7 chunks of 222 (the last 219), rows = 32
  rows42    3 x 700 x 48      rows = 42, 4 idle threads
  lds_full  2 x 300 x 2048    rows = 1, red[2][2048] exactly full
  idle64    1 x 27 x 1536     G = 192: 64 idle threads, one short chunk
  lanes256  2 x 257 x 8       G = 1: 256 voxel lanes for chunks of 129 and 128 voxels
  v1        1 x 1 x 16        V = 1: rstd = 1 / sqrt(eps), z = 0, dx = 0
  chunks65  1 x 16385 x 8     65 chunks: the lane wrap of inorm_finalize_kernel
  empty1    7 x 75009 x 8     293 chunks of 257 per sample, the last one of each sample owns no voxel
  empty7    1 x 524289 x 8    2048 chunks of 257, the last 7 empty; four k0 passes of inorm_finalize_kernel
  offsets   2 x 4099 x 16     17 chunks; the 4 sigma offsets and the constant channel at C = 16
The voxels-per-lane counts of these cases cover every residue modulo UN = 4 (asserted).

Stages and bounds (u = 2^-24; n_k the voxel count of chunk k; S|t| the fp64 sum of |t| over the chunk):
  1 lci_inorm_reduce forward partials: each (b, sum, c, chunk) entry against the fp64 chunk sum of x and of x^2,
    |err| <= n_k u S|t| (first-order worst case of an f32 sum of n_k terms in any order; x^2 of a bf16 is exact in f32);
    an empty chunk must be exactly 0.
  2 lci_inorm_finalize modes 0 and 1 against the same arithmetic in fp64 over the partials the kernel wrote, and over
    synthetic partials p1 = chunk (0.5 + 0.1 randn), p2 = chunk (2 + 0.1 rand) with nchunk = 1, 63, 64, 65, 512, 513,
    683 and 2048 (C = 10 there: the last workgroup has two waves past B C): means |err| <= 2^-23 |ref| + 1e-30, rstd
    2^-22 relative.
  3 lci_inorm_apply forward, act 0 and 1: bitwise bf16(lrelu((x - mean) * rstd)) of the torch f32 restatement from the
    kernel's own stats (subtract, then multiply: nothing to contract), and per element against fp64 from the fp64 stats
    of x: |err| <= 2^-8 |ref| + A. Derivation of A: the chunk partials carry at most n_max u S|t| each (stage 1), so
    after the f64 combine and the division by V
        dmean <= 2^-23 |m| + n_max u E|x|                       (the f32 rounding of the mean included)
        dvar  <= n_max u (E[x^2] + 2 |m| E|x|)                  (var = E[x^2] - m^2, m before its rounding)
        rho = drstd / rstd <= 2^-22 + dvar / (2 (var + eps))    (rstd = (var + eps)^-1/2)
    and n = (x - mean) rstd moves by a_n = rstd dmean + |nhat| (rho + 2^-22) (2^-22: the two f32 roundings of the
    subtract and the multiply, with room). The bf16 rounding acts on the computed value, so
        A = (1 + 2^-8) s a_n,   s = slope where the mask is set, else 1.
  4 backward, act 0 and 1: lci_inorm_reduce partials with dz against fp64 sums of dn and dn n (n in fp64 from the
    kernel's stats), |err| <= (n_k + 4) u S|t| (4: the roundings of n, of dz slope and of the product); the mode-1
    coefficients as stage 2; lci_inorm_apply backward per element against rstd (dn - c1 - n c2) in fp64 from the
    kernel's own stats and coefficients, |err| <= 2^-8 |ref| + 2^-20 rstd (|dn| + |c1| + |n c2|); and end to end
    against the fp64 adjoint of the whole op, with the propagated allowance
        dc1 <= (n_max + 4) u E|dn| + 2^-23 |c1|
        dc2 <= (n_max + 4) u E|dn nhat| + 2^-23 |c2| + rstd dmean E|dn| + (rho + 2^-22) E|dn nhat|   (E[|dn| a_n])
        |err| <= 2^-8 |ref| + (1 + 2^-8) (rho |ref| + rstd (dc1 + a_n |c2| + |nhat| dc2)
                                          + 2^-20 rstd (|dn| + |c1| + |nhat c2|)).
  5 lci_inorm_apply_res, both modes, at rows21, rows42, lds_full, lanes256: bitwise the torch restatement that rounds
    to bf16 after the norm, after the add and after the LeakyReLU; y has its own per-sample statistics, so a kernel
    that read another row of stats_y (or stats in its place) cannot match.
  6 BatchNorm + ReLU at (V, C) = (630, 96), (35, 8), (2574, 64), (300, 2048), (75009, 8), dy f32 and bf16,
    w = 1 + 0.2 randn with w[1] = -0.7, b = 0.2 randn: lci_bn_relu_fwd bitwise the torch f32 restatement
    relu(((x - mean) * rstd) * w + b) (it was not before this test: HIP's __fmul_rn / __fadd_rn are plain * and +,
    the compiler fused them, and y was one f32 ulp off in 8715 of 60480 elements at bn96; csrc/norm.hip bn_affine now
    keeps the product and the sum apart in all three kernels) and per element against fp64,
    |err| <= |w| a_n + 2^-22 (|nhat w| + |b|);
    the lci_bn_relu_bwd_reduce partials as stage 4; lci_bn_relu_bwd_apply per element against fp64 from the kernel's
    stats and coefficients (2^-8 |ref| + 2^-20 rstd |w| (|g| + |m1| + |n m2|)) and end to end (stage 4's allowance
    times |w|); dW = coef[1] V and db = coef[0] V formed in f32 on the device as kernels._BatchNormReLU does, against
    the fp64 sums of g nhat and g: V dc2 + 2^-23 |ref| and V dc1 + 2^-23 |ref|.
  7 exact: two runs over differently pre-filled outputs (NaN, 3.0) agree bit for bit at every stage; the last sample
    repacked as B = 1 gives that sample's stats, z, coefficients and dx bit for bit where nchunk is unchanged.
  8 host checks: C = 12, C = 2056, V = 0, an x pointer offset by 8 bytes (every entry point), dz of lci_inorm_reduce
    offset by 8 bytes, and w, b, coef of lci_bn_relu_* offset by 4 bytes each raise LciError and leave the
    NaN-pre-filled outputs untouched; nothing is launched.

Measured on an MI355X: the largest per-element error of each stage as a fraction of its allowance (part: forward
partials; st: stats from the kernel's partials; z: forward output against fp64; pb: backward partials; cf: mode-1
coefficients; dxk: dx against fp64 of the kernel's own stats and coefficients; dx: dx end to end; rz / rdx: what the
bf16 rounding of the exact fp64 value alone gives against the allowance of z / dx, computed on the CPU; z0 / z1 and
a0 / a1: act 0 / 1).
case       part    st    z0   rz0    z1   rz1 | a0:pb    cf   dxk    dx   rdx | a1:pb    cf   dxk    dx   rdx
rows21    0.020 0.483 0.981 0.981 0.981 0.981 | 0.009 0.491 0.995 0.980 0.980 | 0.013 0.418 0.996 0.978 0.978
chunks7   0.024 0.442 0.983 0.983 0.987 0.987 | 0.007 0.471 0.994 0.983 0.983 | 0.017 0.377 0.995 0.980 0.980
rows42    0.029 0.460 0.983 0.983 0.984 0.984 | 0.010 0.478 0.995 0.982 0.982 | 0.018 0.414 0.994 0.986 0.986
lds_full  0.072 0.487 0.992 0.992 0.991 0.991 | 0.036 0.493 0.996 0.989 0.989 | 0.068 0.490 0.996 0.991 0.991
idle64    0.126 0.481 0.992 0.992 0.986 0.986 | 0.091 0.480 0.994 0.987 0.987 | 0.150 0.481 0.993 0.986 0.986
lanes256  0.036 0.342 0.962 0.962 0.962 0.962 | 0.023 0.385 0.976 0.957 0.957 | 0.057 0.466 0.970 0.933 0.933
v1        0.000 0.175 0.000 0.000 0.000 0.000 | 0.000 0.000 0.000 0.000 0.000 | 0.000 0.000 0.000 0.000 0.000
chunks65  0.062 0.286 0.973 0.973 0.967 0.967 | 0.022 0.475 0.996 0.986 0.986 | 0.040 0.374 0.994 0.983 0.983
empty1    0.092 0.480 0.982 0.982 0.983 0.983 | 0.025 0.488 0.996 0.986 0.986 | 0.054 0.387 0.996 0.987 0.987
empty7    0.086 0.367 0.974 0.974 0.967 0.967 | 0.051 0.480 0.996 0.986 0.986 | 0.106 0.385 0.996 0.987 0.987
offsets   0.050 0.391 0.984 0.984 0.984 0.984 | 0.016 0.441 0.995 0.984 0.984 | 0.032 0.376 0.995 0.971 0.971
BatchNorm + ReLU (y: the f32 forward against fp64; dw, db: the parameter gradients)
case      dy         y     pb     cf    dxk     dx    rdx     dw     db
bn96      f32    0.011  0.016  0.396  0.986  0.966  0.966  0.002  0.009
bn96      bf16   0.011  0.012  0.471  0.991  0.977  0.977  0.003  0.005
bn8       f32    0.031  0.072  0.375  0.930  0.916  0.916  0.024  0.043
bn8       bf16   0.031  0.052  0.315  0.966  0.937  0.937  0.008  0.000
bn64      f32    0.011  0.018  0.429  0.995  0.977  0.977  0.002  0.006
bn64      bf16   0.011  0.016  0.455  0.996  0.973  0.973  0.003  0.004
bn2048    f32    0.037  0.043  0.480  0.996  0.988  0.988  0.014  0.027
bn2048    bf16   0.037  0.039  0.481  0.996  0.985  0.985  0.013  0.009
bn8_long  f32    0.014  0.256  0.428  0.996  0.980  0.980  0.005  0.001
bn8_long  bf16   0.014  0.216  0.375  0.996  0.983  0.983  0.005  0.004
z and dx equal the bf16 rounding of the exact value to three digits: the kernels add nothing visible to that one
rounding; the f32 partials use 1 - 26 % of their first-order bound, the f64 combine sits at the f32 rounding of its
result (under one half). Every bitwise check held (z, y, the residual tail, two pre-fills, the sample repack); the
synthetic finalize cases measured 0.14 - 0.48.
"""
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64            # guard-band elements on either side (128 B of bf16, 256 B of f32: keeps the 16-byte alignment)
SENTINEL = -7.0       # exact in bf16 and f32
U24 = 2.0 ** -24
U_BF16 = 2.0 ** -8
EPS = 1e-5
EPS32 = torch.tensor(EPS, dtype=F32).item()       # the float the entry points receive
SLOPE = 0.01
SLOPE32 = torch.tensor(SLOPE, dtype=F32)
FILLS = {"nan": float("nan"), "three": 3.0}
UN = 4                # csrc/norm.hip inorm_reduce_kernel's unroll

INORM = {
    "rows21": (2, 990, 96), "chunks7": (1, 1551, 64), "rows42": (3, 700, 48), "lds_full": (2, 300, 2048),
    "idle64": (1, 27, 1536), "lanes256": (2, 257, 8), "v1": (1, 1, 16), "chunks65": (1, 16385, 8),
    "empty1": (7, 75009, 8), "empty7": (1, 524289, 8), "offsets": (2, 4099, 16),
}
# what each case is there for, as values of _regime (asserted on the device's lci_inorm_chunks)
REGIME = {
    "rows21": dict(rows=21, idle=4, nchunk=4, chunk=248, empty=0),
    "chunks7": dict(rows=32, idle=0, nchunk=7, chunk=222, last=219),
    "rows42": dict(G=6, rows=42, idle=4),
    "lds_full": dict(G=256, rows=1, idle=0, lds=2048),
    "idle64": dict(G=192, rows=1, idle=64, nchunk=1, chunk=27),
    "lanes256": dict(G=1, rows=256, nchunk=2, chunk=129, last=128),
    "v1": dict(nchunk=1, chunk=1),
    "chunks65": dict(nchunk=65, empty=0),
    "empty1": dict(nchunk=293, chunk=257, empty=1),
    "empty7": dict(nchunk=2048, chunk=257, empty=7),
    "offsets": dict(G=2, rows=128, nchunk=17),
}
RES = ("rows21", "rows42", "lds_full", "lanes256")
BN = {"bn96": (630, 96), "bn8": (35, 8), "bn64": (2574, 64), "bn2048": (300, 2048), "bn8_long": (75009, 8)}


# ------------------------------------------------------------------------------------------------ restated arithmetic
def _chunks(V, B):
    """lci_inorm_chunks: about 2048 workgroups in total, at least 256 voxels per chunk."""
    return max(1, min(-(-2048 // B), -(-V // 256)))


def _regime(B, V, C, nchunk):
    G = C // 8
    rows = 256 // G
    chunk = -(-V // nchunk)
    live = -(-V // chunk)                      # chunks that own a voxel
    return dict(G=G, rows=rows, idle=256 - G * rows, lds=rows * C, nchunk=nchunk, chunk=chunk, empty=nchunk - live,
                last=V - (live - 1) * chunk)


def _chunk_counts(V, nchunk):
    chunk = -(-V // nchunk)
    return (V - torch.arange(nchunk) * chunk).clamp(0, chunk)


def _lane_counts(B, V, C, nchunk):
    """The number of voxels every live voxel lane r < rows of every chunk sums (v0 + r, v0 + r + rows, ...)."""
    rows = 256 // (C // 8)
    n = _chunk_counts(V, nchunk)[:, None] - torch.arange(rows)[None]
    return (-(-n.clamp_min(0) // rows)).flatten()


def _chunk_sums(t, nchunk):
    """t (B, V, C) fp64 -> (B, C, nchunk): the sum over every chunk's voxels."""
    B, V, C = t.shape
    chunk = -(-V // nchunk)
    tp = torch.cat([t, t.new_zeros(B, nchunk * chunk - V, C)], 1)
    return tp.view(B, nchunk, chunk, C).sum(2).permute(0, 2, 1)


def _finalize_ref(part, V, mode):
    """inorm_finalize_kernel's arithmetic in fp64 over part (B, 2, C, nchunk) -> (B, 2, C)."""
    s = part.double().sum(-1) / V
    if mode == 1:
        return s
    return torch.stack([s[:, 0], 1.0 / torch.sqrt((s[:, 1] - s[:, 0] ** 2).clamp_min(0.0) + EPS32)], 1)


def _lrelu32(n, act):
    return torch.where(n < 0, n * SLOPE32, n) if act else n


def _make_x(B, V, C, seed, const=True):
    g = torch.Generator().manual_seed(seed)
    sigma = torch.linspace(0.25, 3.0, C)[torch.randperm(C, generator=g)]
    mu = sigma * torch.linspace(-4.0, 4.0, C)[torch.randperm(C, generator=g)]
    x = (torch.randn(B, V, C, generator=g) * sigma + mu).to(BF16).float()
    if const and C >= 16:
        x[..., C // 2] = 1.5
    return x, g


def _stats64(x):
    """fp64 mean, var, rstd (B, 1, C) and nhat of x (B, V, C)."""
    xd = x.double()
    m = xd.mean(1, keepdim=True)
    var = ((xd - m) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return m, var, rstd, (xd - m) * rstd


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """x, dz (B, V, C) f32 holding bf16 values; computed once, never modified."""
    B, V, C = INORM[name]
    x, g = _make_x(B, V, C, 4000 + list(INORM).index(name))
    nhat = _stats64(x)[3]
    dz = (torch.randn(B, V, C, generator=g).double() + 0.5 + 0.25 * nhat).to(BF16).float()
    return x, dz


def _allow(x, n_max):
    """The propagated stats allowances of the module docstring for x (B, V, C): dict of (B, 1, C) fp64 tensors and
    nhat."""
    xd = x.double()
    m, var, rstd, nhat = _stats64(x)
    e1, e2 = xd.abs().mean(1, keepdim=True), (xd * xd).mean(1, keepdim=True)
    dmean = 2.0 ** -23 * m.abs() + n_max * U24 * e1
    rho = 2.0 ** -22 + 0.5 * n_max * U24 * (e2 + 2 * m.abs() * e1) / (var + EPS)
    return dict(m=m, var=var, rstd=rstd, nhat=nhat, dmean=dmean, rho=rho,
                a_n=rstd * dmean + nhat.abs() * (rho + 2.0 ** -22))


def _bwd_ref_and_allow(al, dn, n_max):
    """The fp64 adjoint rstd (dn - c1 - nhat c2) of the normalisation for the masked cotangent dn, its coefficients,
    and the end-to-end allowance of the module docstring (without the leading 2^-8 |ref|)."""
    rstd, nhat, rho, a_n = al["rstd"], al["nhat"], al["rho"], al["a_n"]
    c1, c2 = dn.mean(1, keepdim=True), (dn * nhat).mean(1, keepdim=True)
    e1, e2 = dn.abs().mean(1, keepdim=True), (dn * nhat).abs().mean(1, keepdim=True)
    dc1 = (n_max + 4) * U24 * e1 + 2.0 ** -23 * c1.abs()
    dc2 = (n_max + 4) * U24 * e2 + 2.0 ** -23 * c2.abs() + rstd * al["dmean"] * e1 + (rho + 2.0 ** -22) * e2
    ref = rstd * (dn - c1 - nhat * c2)
    extra = (1 + U_BF16) * (rho * ref.abs() + rstd * (dc1 + a_n * c2.abs() + nhat.abs() * dc2)
                            + 2.0 ** -20 * rstd * (dn.abs() + c1.abs() + (nhat * c2).abs()))
    return ref, extra, (c1, c2, dc1, dc2)


def _frac(x, ref, allowed):
    """Largest |x - ref| / allowed; a NaN, or any error where nothing is allowed, gives inf."""
    err = (x.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    allowed = allowed.expand_as(err)
    if (err[allowed == 0] != 0).any():
        return math.inf
    return (err / allowed.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------------------------------------ device side
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


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


def _lib():
    from long_context_biomedical_imaging_amd import _lib as lib
    return lib


def _device_stats(xd, B, V, C, fill, st):
    """lci_inorm_reduce + lci_inorm_finalize (mode 0) of the device view xd: (part, stats) as _Out."""
    lib = _lib()
    part = _Out((B, 2, C, lib.load().lci_inorm_chunks(V, B)), F32, fill)
    stats = _Out((B, 2, C), F32, fill)
    lib.call("lci_inorm_reduce", xd.ptr(), None, None, part.ptr(), V, B, C, 0, SLOPE, st)
    lib.call("lci_inorm_finalize", part.ptr(), stats.ptr(), V, B, C, 0, EPS, st)
    return part, stats


def _pipeline(x, dz, act, fill):
    """reduce -> finalize(0) -> apply -> reduce(dz) -> finalize(1) -> apply(dz), each stage reading what the one
    before it wrote; every output back on the CPU."""
    lib = _lib()
    B, V, C = x.shape
    xd, dzd = _In(x), _In(dz)
    st = lib.stream_of(xd.view)
    nch = lib.load().lci_inorm_chunks(V, B)
    o = dict(part=_Out((B, 2, C, nch), F32, fill), stats=_Out((B, 2, C), F32, fill), z=_Out((B, V, C), BF16, fill),
             partb=_Out((B, 2, C, nch), F32, fill), coef=_Out((B, 2, C), F32, fill), dx=_Out((B, V, C), BF16, fill))
    lib.call("lci_inorm_reduce", xd.ptr(), None, None, o["part"].ptr(), V, B, C, act, SLOPE, st)
    lib.call("lci_inorm_finalize", o["part"].ptr(), o["stats"].ptr(), V, B, C, 0, EPS, st)
    lib.call("lci_inorm_apply", xd.ptr(), None, o["stats"].ptr(), None, o["z"].ptr(), V, B, C, act, SLOPE, st)
    lib.call("lci_inorm_reduce", xd.ptr(), dzd.ptr(), o["stats"].ptr(), o["partb"].ptr(), V, B, C, act, SLOPE, st)
    lib.call("lci_inorm_finalize", o["partb"].ptr(), o["coef"].ptr(), V, B, C, 1, EPS, st)
    lib.call("lci_inorm_apply", xd.ptr(), dzd.ptr(), o["stats"].ptr(), o["coef"].ptr(), o["dx"].ptr(), V, B, C, act,
             SLOPE, st)
    torch.cuda.synchronize()
    out = {k: v.view.cpu() for k, v in o.items()}
    out["intact"] = all(v.guards_intact() for v in o.values())
    out["finite"] = all(bool(torch.isfinite(v.view).all()) for v in o.values())
    out["nchunk"] = nch
    return out


@functools.lru_cache(maxsize=None)
def _run(name, act, fill="nan", sample=None):
    x, dz = _inputs(name)
    if sample is not None:
        x, dz = x[sample:sample + 1], dz[sample:sample + 1]
    return _pipeline(x, dz, act, FILLS[fill])


STAGES = ("part", "stats", "z", "partb", "coef", "dx")


# ------------------------------------------------------------------------------------------------ instance norm
@gpu
@pytest.mark.parametrize("name", list(INORM))
def test_inorm_regime(name):
    """The case reaches the thread layout and chunking it is there for, on the device's lci_inorm_chunks."""
    B, V, C = INORM[name]
    nch = _lib().load().lci_inorm_chunks(V, B)
    assert nch == _chunks(V, B)
    got = _regime(B, V, C, nch)
    assert {k: got[k] for k in REGIME[name]} == REGIME[name], got
    assert got["lds"] <= 2048


def test_inorm_cases_cover_every_unroll_residue():
    """The voxels-per-lane counts of the cases cover every residue modulo UN, residue 0 by a lane with UN or more."""
    seen = set()
    for B, V, C in INORM.values():
        n = _lane_counts(B, V, C, _chunks(V, B))
        seen |= {int(r) for r in (n[n > 0] % UN).unique()}
    assert seen == set(range(UN)), seen
    n = _lane_counts(*INORM["rows21"], 4)
    assert set(n.unique().tolist()) == {11, 12}


@gpu
@pytest.mark.parametrize("name", list(INORM))
def test_inorm_forward_stages_vs_fp64(name):
    """Stages 1 to 3 of the module docstring (partials, stats, z for act 0 and 1)."""
    B, V, C = INORM[name]
    x, _ = _inputs(name)
    xd = x.double()
    fails, row = [], {}
    for act in (0, 1):
        out = _run(name, act)
        nch = out["nchunk"]
        n_k = _chunk_counts(V, nch).double()
        if not out["intact"]:
            fails.append(f"act {act}: a guard band was written")
        if not out["finite"]:
            fails.append(f"act {act}: non-finite entries left")
        # stage 1
        ref = torch.stack([_chunk_sums(xd, nch), _chunk_sums(xd * xd, nch)], 1)
        bound = torch.stack([_chunk_sums(xd.abs(), nch), _chunk_sums(xd * xd, nch)], 1) * n_k * U24
        row["part"] = _frac(out["part"], ref, bound)
        empty = n_k == 0
        if empty.any() and _bits(out["part"][..., empty]).any():
            fails.append(f"act {act}: an empty chunk's partial is not zero")
        # stage 2, over the partials the kernel wrote
        sref = _finalize_ref(out["part"], V, 0)
        fm = _frac(out["stats"][:, 0], sref[:, 0], 2.0 ** -23 * sref[:, 0].abs() + 1e-30)
        fr = _frac(out["stats"][:, 1], sref[:, 1], 2.0 ** -22 * sref[:, 1])
        row["st"] = max(fm, fr)
        # stage 3: bitwise the f32 restatement from the kernel's stats, and per element against fp64
        mu, rs = out["stats"][:, 0:1], out["stats"][:, 1:2]
        n32 = (x - mu) * rs
        z32 = _lrelu32(n32, act).to(BF16)
        if not torch.equal(_bits(out["z"]), _bits(z32)):
            bad = (_bits(out["z"]) != _bits(z32)).sum().item()
            fails.append(f"act {act}: z differs from the f32 restatement at {bad} elements")
        al = _allow(x, _regime(B, V, C, nch)["chunk"])
        s = torch.where(n32 < 0, SLOPE32.double(), 1.0) if act else torch.ones(())
        zref = al["nhat"] * s
        A = (1 + U_BF16) * s * al["a_n"]
        row[f"z{act}"] = _frac(out["z"], zref, U_BF16 * zref.abs() + A)
        row[f"rz{act}"] = _frac(zref.to(BF16), zref, U_BF16 * zref.abs() + A)
        if C >= 16 and _bits(out["z"][..., C // 2]).any():
            fails.append(f"act {act}: z of the constant channel is not exactly +0")
        for k in ("part", "st", f"z{act}"):
            if not row[k] <= 1.0:
                fails.append(f"act {act}: {k} error {row[k]:.3f} x the allowance")
    if V == 1:
        assert torch.equal(out["stats"][:, 1], torch.full((B, C), 1.0 / math.sqrt(EPS32)).float())
    print(f"\nTABLE fwd {name:<9} part={row['part']:.3f} st={row['st']:.3f} z0={row['z0']:.3f} rz0={row['rz0']:.3f} "
          f"z1={row['z1']:.3f} rz1={row['rz1']:.3f}")
    assert not fails, "\n".join(fails)


@gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("name", list(INORM))
def test_inorm_backward_stages_vs_fp64(name, act):
    """Stage 4 of the module docstring."""
    B, V, C = INORM[name]
    x, dz = _inputs(name)
    out = _run(name, act)
    nch = out["nchunk"]
    n_k = _chunk_counts(V, nch).double()
    fails, row = [], {}
    mu, rs = out["stats"][:, 0:1], out["stats"][:, 1:2]
    n32 = (x - mu) * rs
    s = torch.where(n32 < 0, SLOPE32.double(), 1.0) if act else torch.ones((), dtype=F64)
    nk = (x.double() - mu.double()) * rs.double()            # n in fp64 from the kernel's own stats
    dn = dz.double() * s
    # the partials
    ref = torch.stack([_chunk_sums(dn, nch), _chunk_sums(dn * nk, nch)], 1)
    bound = torch.stack([_chunk_sums(dn.abs(), nch), _chunk_sums((dn * nk).abs(), nch)], 1) * (n_k + 4) * U24
    bound = torch.where(n_k == 0, torch.zeros(()), bound)
    row["pb"] = _frac(out["partb"], ref, bound)
    # the coefficients over the partials the kernel wrote
    cref = _finalize_ref(out["partb"], V, 1)
    row["cf"] = _frac(out["coef"], cref, 2.0 ** -23 * cref.abs() + 1e-30)
    # dx from the kernel's own stats and coefficients
    c1, c2 = out["coef"][:, 0:1].double(), out["coef"][:, 1:2].double()
    rsd = rs.double()
    ref = rsd * (dn - c1 - nk * c2)
    row["dxk"] = _frac(out["dx"], ref, U_BF16 * ref.abs() + 2.0 ** -20 * rsd * (dn.abs() + c1.abs() + (nk * c2).abs()))
    # end to end
    al = _allow(x, _regime(B, V, C, nch)["chunk"])
    ref, extra, _ = _bwd_ref_and_allow(al, dn, _regime(B, V, C, nch)["chunk"])
    row["dx"] = _frac(out["dx"], ref, U_BF16 * ref.abs() + extra)
    row["rdx"] = _frac(ref.to(BF16), ref, U_BF16 * ref.abs() + extra)
    if C >= 16 and _bits(n32[..., C // 2]).any():
        fails.append("n of the constant channel is not exactly +0")
    for k in ("pb", "cf", "dxk", "dx"):
        if not row[k] <= 1.0:
            fails.append(f"{k} error {row[k]:.3f} x the allowance")
    print(f"\nTABLE bwd {name:<9} act={act} pb={row['pb']:.3f} cf={row['cf']:.3f} dxk={row['dxk']:.3f} "
          f"dx={row['dx']:.3f} rdx={row['rdx']:.3f}")
    assert not fails, "\n".join(fails)


@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nchunk", [1, 63, 64, 65, 512, 513, 683, 2048])
def test_inorm_finalize_synthetic_partials(nchunk, mode):
    """lci_inorm_finalize over synthetic partials, so every lane-wrap and k0-pass count is reached without a large
    input. C = 10 (the entry point sets no multiple): B C = 10 or 30 waves, the last workgroup has two waves that
    return."""
    lib = _lib()
    B = 3 if nchunk == 683 else 1
    V = 2048 * 256 if nchunk == 683 else nchunk * 256 - 3
    C = 10
    assert lib.load().lci_inorm_chunks(V, B) == nchunk == _chunks(V, B)
    g = torch.Generator().manual_seed(5000 + nchunk)
    chunk = V / nchunk
    part = torch.stack([chunk * (0.5 + 0.1 * torch.randn(B, C, nchunk, generator=g)),
                        chunk * (2.0 + 0.1 * torch.rand(B, C, nchunk, generator=g))], 1).float()
    ref = _finalize_ref(part, V, mode)
    res = []
    for fill in FILLS.values():
        pd = _In(part, F32)
        o = _Out((B, 2, C), F32, fill)
        lib.call("lci_inorm_finalize", pd.ptr(), o.ptr(), V, B, C, mode, EPS, lib.stream_of(pd.view))
        torch.cuda.synchronize()
        assert o.guards_intact()
        res.append(o.view.cpu())
    assert torch.equal(_bits(res[0]), _bits(res[1])), "two runs differ"
    fm = _frac(res[0][:, 0], ref[:, 0], 2.0 ** -23 * ref[:, 0].abs() + 1e-30)
    fr = _frac(res[0][:, 1], ref[:, 1], 2.0 ** -22 * ref[:, 1] if mode == 0 else 2.0 ** -23 * ref[:, 1].abs() + 1e-30)
    print(f"\nTABLE fin nchunk={nchunk} mode={mode} first={fm:.3f} second={fr:.3f}")
    assert fm <= 1.0 and fr <= 1.0, (fm, fr)


@gpu
@pytest.mark.parametrize("name", list(INORM))
def test_inorm_two_runs_and_sample_repack(name):
    """Stage 7: NaN- and 3.0-pre-filled outputs give the same bits at every stage; the last sample as a B = 1 problem
    gives that sample's stats, z, coefficients and dx bit for bit where nchunk is unchanged."""
    B, V, C = INORM[name]
    a, b = _run(name, 1), _run(name, 1, "three")
    assert b["intact"] and b["finite"]
    for k in STAGES:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{k}: two runs differ"
    if B > 1 and _chunks(V, 1) == _chunks(V, B):
        s = _run(name, 1, "nan", B - 1)
        assert s["intact"] and s["nchunk"] == a["nchunk"]
        for k in STAGES:
            assert torch.equal(_bits(s[k]), _bits(a[k][-1:])), f"{k}: the B = 1 repack of a sample differs"
    else:
        assert B == 1 or name == "empty1"


# ------------------------------------------------------------------------------------------------ residual tail
@gpu
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("name", RES)
def test_inorm_apply_res_bitwise(name, pre):
    """Stage 5: lci_inorm_apply_res against the torch restatement with its three bf16 roundings, from the stats the
    kernels wrote for x and (pre) for y; two pre-fills agree."""
    lib = _lib()
    B, V, C = INORM[name]
    x, _ = _inputs(name)
    y, _ = _make_x(B, V, C, 4500 + list(INORM).index(name), const=False)
    res = []
    for fill in FILLS.values():
        xd, yd = _In(x), _In(y)
        st = lib.stream_of(xd.view)
        _, sx = _device_stats(xd, B, V, C, fill, st)
        _, sy = _device_stats(yd, B, V, C, fill, st)
        o = _Out((B, V, C), BF16, fill)
        lib.call("lci_inorm_apply_res", xd.ptr(), sx.ptr(), yd.ptr(), sy.ptr() if pre else None, o.ptr(), V, B, C,
                 SLOPE, st)
        torch.cuda.synchronize()
        assert o.guards_intact() and torch.isfinite(o.view).all()
        res.append((o.view.cpu(), sx.view.cpu(), sy.view.cpu()))
    out, sx, sy = res[0]
    assert torch.equal(_bits(out), _bits(res[1][0])), "two runs differ"
    if B > 1:
        assert not torch.equal(sy[0], sy[1]) and not torch.equal(sx, sy)
    n = ((x - sx[:, 0:1]) * sx[:, 1:2]).to(BF16).float()
    r = ((y - sy[:, 0:1]) * sy[:, 1:2]).to(BF16).float() if pre else y
    t = (n + r).to(BF16).float()
    ref = torch.where(t > 0, t, t * SLOPE32).to(BF16)
    bad = (_bits(out) != _bits(ref)).sum().item()
    assert bad == 0, f"{bad} elements differ from the restatement"


# ------------------------------------------------------------------------------------------------ BatchNorm + ReLU
@functools.lru_cache(maxsize=None)
def _bn_inputs(name):
    V, C = BN[name]
    x, g = _make_x(1, V, C, 6000 + list(BN).index(name))
    w = 1 + 0.2 * torch.randn(C, generator=g)
    w[1] = -0.7
    b = 0.2 * torch.randn(C, generator=g)
    dy = (torch.randn(1, V, C, generator=g).double() + 0.5 + 0.25 * _stats64(x)[3]).float()
    return x, w, b, dy


def _bn_pipeline(name, dy_f32, fill):
    lib = _lib()
    V, C = BN[name]
    x, w, b, dy = _bn_inputs(name)
    if not dy_f32:
        dy = dy.to(BF16).float()
    xd, wd, bd, dyd = _In(x), _In(w, F32), _In(b, F32), _In(dy, F32 if dy_f32 else BF16)
    st = lib.stream_of(xd.view)
    nch = lib.load().lci_inorm_chunks(V, 1)
    part, stats = _device_stats(xd, 1, V, C, fill, st)
    o = dict(part=part, stats=stats, y=_Out((V, C), F32, fill), partb=_Out((2, C, nch), F32, fill),
             coef=_Out((1, 2, C), F32, fill), dx=_Out((V, C), BF16, fill))
    lib.call("lci_bn_relu_fwd", xd.ptr(), stats.ptr(), wd.ptr(), bd.ptr(), o["y"].ptr(), V, C, st)
    lib.call("lci_bn_relu_bwd_reduce", xd.ptr(), dyd.ptr(), int(dy_f32), stats.ptr(), wd.ptr(), bd.ptr(),
             o["partb"].ptr(), V, C, st)
    lib.call("lci_inorm_finalize", o["partb"].ptr(), o["coef"].ptr(), V, 1, C, 1, EPS, st)
    lib.call("lci_bn_relu_bwd_apply", xd.ptr(), dyd.ptr(), int(dy_f32), stats.ptr(), o["coef"].ptr(), wd.ptr(),
             bd.ptr(), o["dx"].ptr(), V, C, st)
    dw, db = o["coef"].view[0, 1] * V, o["coef"].view[0, 0] * V          # as kernels._BatchNormReLU.backward
    torch.cuda.synchronize()
    out = {k: v.view.cpu() for k, v in o.items()}
    out.update(dw=dw.cpu(), db=db.cpu(), nchunk=nch, dy=dy, intact=all(v.guards_intact() for v in o.values()),
               finite=all(bool(torch.isfinite(v.view).all()) for v in o.values()))
    return out


@gpu
@pytest.mark.parametrize("dy_f32", [True, False])
@pytest.mark.parametrize("name", list(BN))
def test_bn_relu_stages_vs_fp64(name, dy_f32):
    """Stage 6 of the module docstring."""
    V, C = BN[name]
    x, w, b, _ = _bn_inputs(name)
    out, again = _bn_pipeline(name, dy_f32, FILLS["nan"]), _bn_pipeline(name, dy_f32, FILLS["three"])
    dy = out["dy"]
    nch = out["nchunk"]
    assert nch == _chunks(V, 1)
    n_max = -(-V // nch)
    n_k = _chunk_counts(V, nch).double()
    fails, row = [], {}
    if not (out["intact"] and again["intact"]):
        fails.append("a guard band was written")
    if not out["finite"]:
        fails.append("non-finite entries left")
    for k in ("part", "stats", "y", "partb", "coef", "dx", "dw", "db"):
        if not torch.equal(_bits(out[k]), _bits(again[k])):
            fails.append(f"{k}: two runs differ")
    x2, xd = x[0], x[0].double()
    mu, rs = out["stats"][0, 0], out["stats"][0, 1]
    n32 = (x2 - mu) * rs
    pre32 = n32 * w + b
    y32 = torch.where(pre32 > 0, pre32, torch.zeros(()))
    if not torch.equal(_bits(out["y"]), _bits(y32)):
        fails.append(f"y differs from the f32 restatement at {(_bits(out['y']) != _bits(y32)).sum().item()} elements")
    mask = (pre32 > 0).double()
    al = {k: v[0] for k, v in _allow(x, n_max).items()}
    wd, bd = w.double(), b.double()
    yref = mask * (al["nhat"] * wd + bd)
    row["y"] = _frac(out["y"], yref, wd.abs() * al["a_n"] + 2.0 ** -22 * ((al["nhat"] * wd).abs() + bd.abs()))
    # backward partials, n in fp64 from the kernel's stats
    nk = (xd - mu.double()) * rs.double()
    g = dy[0].double() * mask
    ref = torch.stack([_chunk_sums(g[None], nch)[0], _chunk_sums((g * nk)[None], nch)[0]])
    bound = torch.stack([_chunk_sums(g.abs()[None], nch)[0], _chunk_sums((g * nk).abs()[None], nch)[0]])
    row["pb"] = _frac(out["partb"], ref, bound * (n_k + 4) * U24)
    cref = _finalize_ref(out["partb"][None], V, 1)
    row["cf"] = _frac(out["coef"], cref, 2.0 ** -23 * cref.abs() + 1e-30)
    m1, m2, rsd = out["coef"][0, 0].double(), out["coef"][0, 1].double(), rs.double()
    ref = (g - m1 - nk * m2) * rsd * wd
    row["dxk"] = _frac(out["dx"], ref, U_BF16 * ref.abs()
                       + 2.0 ** -20 * rsd * wd.abs() * (g.abs() + m1.abs() + (nk * m2).abs()))
    ref, extra, (c1, c2, dc1, dc2) = _bwd_ref_and_allow({k: v[None] for k, v in al.items()}, g[None], n_max)
    ref, extra = ref[0] * wd, extra[0] * wd.abs()
    row["dx"] = _frac(out["dx"], ref, U_BF16 * ref.abs() + extra)
    row["rdx"] = _frac(ref.to(BF16), ref, U_BF16 * ref.abs() + extra)
    dwref, dbref = (g * al["nhat"]).sum(0), g.sum(0)
    row["dw"] = _frac(out["dw"], dwref, V * dc2[0, 0] + 2.0 ** -23 * dwref.abs())
    row["db"] = _frac(out["db"], dbref, V * dc1[0, 0] + 2.0 ** -23 * dbref.abs())
    for k, v in row.items():
        if k != "rdx" and not v <= 1.0:
            fails.append(f"{k} error {v:.3f} x the allowance")
    print(f"\nTABLE bn {name:<9} dy={'f32' if dy_f32 else 'bf16'} " + " ".join(f"{k}={v:.3f}" for k, v in row.items()))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ host checks
HC_B, HC_V, HC_C, HC_CMAX = 1, 5, 16, 2056


def _host_call(entry, bad):
    """One invalid call of `entry` on a 1 x 5 x 16 problem whose buffers are sized for C = 2056; True when it raised
    LciError and every NaN-pre-filled output is untouched."""
    lib = _lib()
    g = torch.Generator().manual_seed(88)
    V, C = bad.get("V", HC_V), bad.get("C", HC_C)
    n = HC_B * HC_V * HC_CMAX
    x, dz, y = (_In(torch.randn(n + 8, generator=g)) for _ in range(3))
    dyf = _In(torch.randn(n + 8, generator=g), F32)
    stats, coef, stats_y, w, b = (_In(torch.rand(2 * HC_CMAX + 8, generator=g) + 0.5, F32) for _ in range(5))
    part = _Out((2 * HC_CMAX,), F32, float("nan"))
    out = _Out((n,), F32, float("nan"))            # f32-sized: holds either output type
    st = lib.stream_of(x.view)
    p = dict(x=x.ptr() + bad.get("x", 0), dz=dz.ptr() + bad.get("dz", 0), w=w.ptr() + bad.get("w", 0),
             b=b.ptr() + bad.get("b", 0), coef=coef.ptr() + bad.get("coef", 0))
    calls = {
        "reduce": lambda: lib.call("lci_inorm_reduce", p["x"], None, None, part.ptr(), V, HC_B, C, 1, SLOPE, st),
        "reduce_bwd": lambda: lib.call("lci_inorm_reduce", p["x"], p["dz"], stats.ptr(), part.ptr(), V, HC_B, C, 1,
                                       SLOPE, st),
        "finalize": lambda: lib.call("lci_inorm_finalize", part.ptr(), out.ptr(), V, HC_B, C, 0, EPS, st),
        "apply": lambda: lib.call("lci_inorm_apply", p["x"], None, stats.ptr(), None, out.ptr(), V, HC_B, C, 1, SLOPE,
                                  st),
        "apply_bwd": lambda: lib.call("lci_inorm_apply", p["x"], p["dz"], stats.ptr(), p["coef"], out.ptr(), V, HC_B,
                                      C, 1, SLOPE, st),
        "apply_res": lambda: lib.call("lci_inorm_apply_res", p["x"], stats.ptr(), y.ptr(), stats_y.ptr(), out.ptr(),
                                      V, HC_B, C, SLOPE, st),
        "bn_fwd": lambda: lib.call("lci_bn_relu_fwd", p["x"], stats.ptr(), p["w"], p["b"], out.ptr(), V, C, st),
        "bn_bwd_reduce": lambda: lib.call("lci_bn_relu_bwd_reduce", p["x"], dyf.ptr(), 1, stats.ptr(), p["w"], p["b"],
                                          part.ptr(), V, C, st),
        "bn_bwd_apply": lambda: lib.call("lci_bn_relu_bwd_apply", p["x"], dyf.ptr(), 1, stats.ptr(), p["coef"],
                                         p["w"], p["b"], out.ptr(), V, C, st),
    }
    with pytest.raises(lib.LciError):
        calls[entry]()
    torch.cuda.synchronize()
    return part.unchanged() and out.unchanged()


WITH_X = ("reduce", "reduce_bwd", "apply", "apply_bwd", "apply_res", "bn_fwd", "bn_bwd_reduce", "bn_bwd_apply")
BN_ENTRIES = ("bn_fwd", "bn_bwd_reduce", "bn_bwd_apply")
HOST = ([(e, "C", 12) for e in WITH_X] + [(e, "C", 2056) for e in WITH_X] + [(e, "V", 0) for e in WITH_X]
        + [("finalize", "V", 0)] + [(e, "x", 8) for e in WITH_X] + [("reduce_bwd", "dz", 8), ("apply_bwd", "dz", 8)]
        + [(e, k, 4) for e in BN_ENTRIES for k in ("w", "b")] + [("bn_bwd_apply", "coef", 4), ("apply_bwd", "coef", 4)])


@gpu
@pytest.mark.parametrize("entry,what,value", HOST, ids=[f"{e}-{k}{v}" for e, k, v in HOST])
def test_norm_host_checks(entry, what, value):
    """Stage 8: the invalid call raises LciError before anything is launched; the outputs keep their NaN pre-fill."""
    assert _host_call(entry, {what: value})


@gpu
@pytest.mark.parametrize("which", ["weight", "bias"])
def test_batch_norm_relu_supported_rejects_misaligned_parameters(which):
    """A BatchNorm parameter that is a view 4 bytes into its storage would fail lci_bn_relu_*'s alignment check:
    kernels.batch_norm_relu_supported says so, and the module keeps the unfused ops."""
    from long_context_biomedical_imaging_amd import kernels
    bn = torch.nn.BatchNorm2d(16).cuda().train()
    x = torch.randn(2, 16, 5, 7, device="cuda").to(BF16).to(memory_format=torch.channels_last)
    assert kernels.batch_norm_relu_supported(x, bn)
    setattr(bn, which, torch.nn.Parameter(torch.ones(17, device="cuda")[1:]))
    assert getattr(bn, which).data_ptr() % 16 == 4
    assert not kernels.batch_norm_relu_supported(x, bn)
