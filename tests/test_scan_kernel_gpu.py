"""GPU: the selective-scan kernels (csrc/mamba.hip: scan_fwd_kernel modes 0 / 1, scan_carry_kernel forward / reverse,
scan_bwd_agg_kernel, scan_bwd_kernel with partials or atomics, scan_param_reduce_kernel) called through the C entry
points lci_selective_scan_fwd / lci_selective_scan_bwd with an explicit chunk length Tc, caller-owned workspaces and
caller-chosen strides, against a plain fp64 per-step loop written here (_reference). The loop is pinned once, on the
CPU, against oracle.selective_scan with autograd in fp64 (test_reference_is_pinned_by_the_oracle, not a GPU test).

Stage quantities (dt' = softplus(delta + delta_bias), or delta + delta_bias with delta_softplus = 0; a_t = exp(dt'_t A);
x_t = a_t x_{t-1} + dt'_t u_t B_t; lambda_t = C_t dy_t + a_{t+1} lambda_{t+1} the adjoint of x_t; chunk c holds the
steps [c Tc, min(L, (c + 1) Tc))):
  sdt[b,c,d]      sum of dt' over chunk c
  xend[b,c,d,n]   the state at the chunk's end when the chunk starts from a zero state
  xinit[b,c]      the true state before the chunk's first step (xinit[c+1] = exp(A sdt[c]) xinit[c] + xend[c], the
                  forward carry's recurrence); xinit[:, 0] is exactly 0
  ckpt[b,k,d,n]   the true state before step 8 k (k = 0: zero), stored in the I/O dtype
  gl[b,c]         a_{t0} lambda_{t0} of the chunk's first step t0 with zero adjoint flowing in from later chunks
                  (scan_bwd_agg_kernel: "local adjoint with zero carry-in from later chunks: Gl = a_{t0} g_{t0}")
  gin[b,c]        the decayed adjoint a lambda flowing into the chunk's last step from the next chunk
                  (scan_carry_kernel reverse: gin[c] = carry; carry = gl[c] + exp(A sdt[c]) carry, chunks from last to
                  first); gin[:, nch - 1] is exactly 0
With Tc < 512 the backward kernel overwrites gin / gl with per-(b, chunk) parameter partials, dA in gin[..., 0:8],
dD in gl[..., 0], d(delta_bias) in gl[..., 1], summed afterwards by scan_param_reduce_kernel: there the partials are
compared with the fp64 per-chunk contributions (so the scan kernel and the reduce kernel are judged separately), and
gl / gin are compared as adjoints only with Tc >= 512, where the backward leaves them alone.

Inputs, one seeded CPU generator per case, rounded to the I/O dtype before either side sees them: u ~ N(0,1),
delta ~ 0.5 N - 1, A = -exp(0.3 N), B, C ~ N(0,1), D ~ N(0,1), delta_bias ~ 0.1 N, dy ~ N(0,1); with
delta_softplus = 0, delta = 0.2 |N| + 0.01.

Cases (CASES; every shape in f32 and in bf16 unless a dtype is named) and the structure each one reaches:
  tc8_l5        Tc 8, L 5, Dx 24, B 1: nch 1, one partial sub-block (L < CKPT), non-null workspaces with one chunk
  tc8_l533      Tc 8, L 533, Dx 24, B 1: nch 67, carry groups G = 9 > PF: the second PF batch of scan_carry_kernel in
                both directions; forward grid of 17 workgroups, the last with 3 live waves; scan_param_reduce_kernel
                with 67 rows over 4 row-blocks (unrolled loop and tail loop)
  tc64_l321     Tc 64, L 64*5+1, Dx 72, B 3: multi-chunk with B > 1, nch 6 < 8 (empty carry groups), last chunk of one
                step, partial second wave, the `chunk >= nch` early return of waves 2, 3 of the second workgroup
  tc64_l569     Tc 64, L 64*9-7, Dx 256, B 1: nch 9, G = 2, partly filled last carry group; 4-wave workgroup, plain dBC
  tc72_l303     Tc 72, L 72*4+15, Dx 264, B 2: short last staging block (8 steps), odd number of 8-step groups in the
                pipelined forward, mid-chunk dB/dC flush and re-zero; Dx > 256: a second workgroup of channels with 3
                fully padded waves, dBC accumulated with global atomics
  tc200_l599    Tc 200, L 200*2+199, Dx 320, B 1: 3 full staging blocks + 8 steps; Dx > 256 with two live workgroups
  tc512_l521    Tc 512, L 512+9, Dx 64, B 2: the Tc >= 512 regime: one wave per workgroup, float atomics for dA / dD /
                d(delta_bias), plain dBC with `single` stores; gl / gin checked as adjoints
  tc520_l4197   Tc 520, L 520*8+37, Dx 72, B 1: the same with atomic dBC (2 workgroups of one wave), nch 9: the
                reverse carry's group structure checked directly on gin
  nosoftplus    f32, Tc 72, L 159, Dx 72, B 2: delta_softplus = 0 in the forward and in the backward (delta_bias null,
                as in test_compat_selective_scan_fn_signature: dt' = delta stays positive, a stable recurrence)
  nullparams    bf16, Tc 64, L 137, Dx 40, B 1: D and delta_bias passed as null pointers
  strided       f32 and bf16, Tc 72, L 159, Dx 72, B 2: u, delta, dy, du, ddelta with token stride Dx + 24; y in the
                first half of a (B, L, 2 Dx) buffer (the yz layout); B and C the column slices [24:32], [32:40] of one
                (B, L, 40) tensor. The pad columns of every input hold NaN.
  one_l37       f32, Tc 64, L 37, Dx 200, B 3: the one-chunk entry, xend = xinit = sdt = null
  one_l343      bf16, Tc 344, L 343, Dx 96, B 2: the same over 5 full staging blocks + 23 steps

Numeric bounds, all against the fp64 loop, which sees the same rounded inputs:
  f32 I/O    rel-L2 <= 1e-4 on y, xend, sdt, xinit, ckpt (the arithmetic of y; test_mamba_gpu.py's forward bound) and
             <= 2e-4 on du, ddelta, dB|dC, dA, dD, d(delta_bias), gl, gin and the parameter partials
             (test_selective_scan_vs_reference_fixture's gradient bound)
  bf16 I/O   rel-L2 <= 5e-3 on y and every gradient (test_scan_long_gpu.py); the f32 workspaces xend, sdt, xinit keep
             1e-4 (no bf16 store is involved); ckpt, a bf16 store of an f32 state like y, 5e-3; ckpt and y also per
             element |err| <= 2^-8 |ref| + 1e-4 max|ref| (one bf16 rounding of the f32 value moves it by at most half
             an ulp, 2^-8 relative with 8 significant bits; the f32 value's own error, which can also flip that
             rounding, moves the result by no more than itself: the second term, the f32 bound)
Each rel-L2 bound is applied to the whole tensor, per sample, and to windows, so that one wrong token at a seam cannot
hide in the norm: for the per-token tensors (y, du, ddelta, dB|dC) the 8 tokens on either side of every chunk boundary,
the first and the last 8 tokens and the last sub-block; for the per-chunk tensors every chunk on its own; for ckpt
every checkpoint on its own. Where the reference of such a group is identically zero the result must be exactly zero.

Exact checks: every output and workspace is a view inside a larger buffer with 64-element sentinel guard bands,
pre-filled with NaN; the guard bands and the pad columns [Dx, stride) of the strided buffers stay bitwise untouched
(what keeps the scan out of the z half of yz) and every in-range entry of y, du, ddelta, xend, sdt, xinit, ckpt, and
with Tc < 512 of the partials, comes out finite. dBC is pre-filled with NaN where lci_selective_scan_bwd_plain_dbc
returns 1 (the no-zero-fill contract: it must come out finite and within bound everywhere) and with zeros where it
returns 0; the function's value is asserted against its rule (one workgroup of min(4 or, with Tc >= 512, 1,
ceil(Dx / 64)) waves holds all channels). The last sample repacked as a B = 1 problem gives y, du, ddelta, xend, xinit,
sdt, ckpt equal to the batched run's slice bit for bit; two runs over differently pre-filled buffers (NaN / 3.0) agree
bit for bit on those tensors and to the allowance of test_selective_scan_one_chunk_path_bitwise (1e-4 max|ref| + 1e-6)
on the atomically summed dBC / dA / dD / d(delta_bias). Host checks: N = 4, chunk = 12, Dx = 1025, a bf16 B slice at a
column offset of 4 elements and a null sdt with two chunks each raise LciError from both entry points and leave every
NaN-pre-filled output untouched.

Measured on an MI355X against fp64: for each quantity the largest rel-L2 of the whole tensor, any sample and any window
(y_el / ck_el: the largest per-element error as a fraction of its allowance; the bf16 rounding of the exact value alone
gives 0.84 .. 0.92 there and 1.7e-3 .. 2.0e-3 rel-L2 on y, ckpt, du, ddelta, so the kernels add nothing visible to it;
"-": not produced or overwritten in that case; 0: exact). Every exact check held bit for bit, every windowed bound was
met as stated, and the atomically summed tensors of two runs agreed within the allowance. dA_p / dD_p / db_p are the
parameter partials. In f32 everything sits at 1e-7 .. 6e-7 against bounds of 1e-4 / 2e-4; in bf16 the gradients summed
in f32 (dBC, dA, d(delta_bias)) carry 5e-4 .. 3e-3 (the recompute starts from bf16 checkpoints), against 5e-3.
Forward side first, then backward side:
case                    y    y_el     sdt    xend   xinit    ckpt   ck_el
tc8_l5_f32           1e-7       -    7e-8    1e-7       0       0       -
tc8_l5_bf16          2e-3    0.88    6e-8    1e-7       0       0    0.00
tc8_l533_f32         1e-7       -    8e-8    2e-7    2e-7    2e-7       -
tc8_l533_bf16        2e-3    0.87    8e-8    2e-7    2e-7    2e-3    0.90
tc64_l321_f32        1e-7       -    1e-7    1e-7    1e-7    1e-7       -
tc64_l321_bf16       2e-3    0.88    1e-7    1e-7    1e-7    2e-3    0.89
tc64_l569_f32        1e-7       -    1e-7    1e-7    1e-7    1e-7       -
tc64_l569_bf16       2e-3    0.90    1e-7    1e-7    1e-7    2e-3    0.91
tc72_l303_f32        1e-7       -    1e-7    1e-7    1e-7    1e-7       -
tc72_l303_bf16       2e-3    0.89    1e-7    1e-7    1e-7    2e-3    0.91
tc200_l599_f32       1e-7       -    2e-7    1e-7    1e-7    1e-7       -
tc200_l599_bf16      2e-3    0.91    2e-7    1e-7    1e-7    2e-3    0.91
tc512_l521_f32       1e-7       -    4e-7    1e-7    1e-7    1e-7       -
tc512_l521_bf16      2e-3    0.90    4e-7    1e-7    1e-7    2e-3    0.91
tc520_l4197_f32      1e-7       -    4e-7    1e-7    1e-7    1e-7       -
tc520_l4197_bf16     2e-3    0.90    4e-7    1e-7    1e-7    2e-3    0.91
nosoftplus_f32       8e-8       -    1e-7    8e-8    9e-8    9e-8       -
nullparams_bf16      2e-3    0.89    1e-7    1e-7    1e-7    2e-3    0.88
strided_f32          1e-7       -    1e-7    1e-7    1e-7    1e-7       -
strided_bf16         2e-3    0.89    1e-7    1e-7    1e-7    2e-3    0.89
one_l37_f32          1e-7       -       -       -       -    1e-7       -
one_l343_bf16        2e-3    0.84       -       -       -    2e-3    0.92
case                   du  ddelta     dBC      dA      dD     ddb    dA_p    dD_p    db_p      gl     gin
tc8_l5_f32           1e-7    1e-7    1e-7    2e-7    6e-8    2e-7    2e-7    6e-8    2e-7       -       -
tc8_l5_bf16          2e-3    2e-3    1e-7    1e-7       0    1e-7    1e-7       0    1e-7       -       -
tc8_l533_f32         1e-7    2e-7    2e-7    2e-7    1e-7    2e-7    3e-7    8e-8    3e-7       -       -
tc8_l533_bf16        2e-3    2e-3    8e-4    1e-3    8e-8    7e-4    2e-3    5e-8    2e-3       -       -
tc64_l321_f32        1e-7    1e-7    1e-7    2e-7    1e-7    2e-7    2e-7    1e-7    2e-7       -       -
tc64_l321_bf16       2e-3    2e-3    1e-3    8e-4    7e-8    5e-4    2e-3    6e-8    1e-3       -       -
tc64_l569_f32        1e-7    2e-7    3e-7    2e-7    1e-7    2e-7    2e-7    1e-7    2e-7       -       -
tc64_l569_bf16       2e-3    2e-3    1e-3    8e-4    6e-8    6e-4    9e-4    6e-8    8e-4       -       -
tc72_l303_f32        1e-7    1e-7    2e-7    2e-7    2e-7    2e-7    2e-7    2e-7    2e-7       -       -
tc72_l303_bf16       2e-3    2e-3    6e-4    9e-4    7e-8    6e-4    1e-3    6e-8    7e-4       -       -
tc200_l599_f32       1e-7    1e-7    2e-7    3e-7    2e-7    3e-7    3e-7    3e-7    3e-7       -       -
tc200_l599_bf16      2e-3    2e-3    5e-4    9e-4    9e-8    7e-4    9e-4    9e-8    8e-4       -       -
tc512_l521_f32       1e-7    2e-7    1e-7    4e-7    5e-7    4e-7       -       -       -    1e-7    1e-7
tc512_l521_bf16      2e-3    2e-3    3e-3    8e-4    2e-7    7e-4       -       -       -    8e-8    8e-8
tc520_l4197_f32      1e-7    1e-7    2e-7    4e-7    4e-7    6e-7       -       -       -    1e-7    1e-7
tc520_l4197_bf16     2e-3    2e-3    7e-4    9e-4    2e-7    6e-4       -       -       -    9e-8    9e-8
nosoftplus_f32       8e-8    1e-7    1e-7    2e-7    1e-7    2e-7    2e-7    1e-7    2e-7       -       -
nullparams_bf16      2e-3    2e-3    1e-3    1e-3    8e-8    5e-4    1e-3    6e-8    9e-4       -       -
strided_f32          1e-7    1e-7    2e-7    2e-7    1e-7    2e-7    2e-7    2e-7    2e-7       -       -
strided_bf16         2e-3    2e-3    6e-4    9e-4    7e-8    5e-4    1e-3    6e-8    8e-4       -       -
one_l37_f32          1e-7    1e-7    1e-7    2e-7    1e-7    2e-7    2e-7    1e-7    2e-7       -       -
one_l343_bf16        2e-3    2e-3    5e-4    1e-3    1e-7    6e-4    1e-3    1e-7    8e-4       -       -
"""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from oracle import selective_scan as oscan

gpu = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
N = 8                 # d_state
CKPT = 8              # csrc/mamba.hip CKPT
GUARD = 64            # guard-band elements on either side (128 B of bf16, 256 B of f32: keeps the 16-byte alignment)
SENTINEL = -7.0       # exact in bf16 and f32
PAD = 24              # extra columns of the strided token rows
R = 24                # dt_rank columns in front of B | C in the strided x_dbl layout
U_BF16 = 2.0 ** -8
FILLS = {"nan": float("nan"), "three": 3.0}
BITWISE = ("y", "du", "ddelta", "xend", "xinit", "sdt", "ckpt")
ATOMIC = ("dBC", "dA", "dD", "ddb")


@dataclasses.dataclass(frozen=True)
class Case:
    Tc: int
    L: int
    Dx: int
    B: int
    dtype: torch.dtype
    softplus: int = 1
    null_D: bool = False       # D passed as a null pointer
    null_bias: bool = False    # delta_bias passed as a null pointer
    strided: bool = False
    null_ws: bool = False      # the one-chunk entry: xend = xinit = sdt = null

    @property
    def nch(self):
        return -(-self.L // self.Tc)

    @property
    def nck(self):
        return -(-self.L // CKPT)

    @property
    def partials(self):        # the backward overwrites gl / gin with parameter partials
        return self.Tc < 512


_SHAPES = {
    "tc8_l5": (8, 5, 24, 1),
    "tc8_l533": (8, 533, 24, 1),
    "tc64_l321": (64, 64 * 5 + 1, 72, 3),
    "tc64_l569": (64, 64 * 9 - 7, 256, 1),
    "tc72_l303": (72, 72 * 4 + 15, 264, 2),
    "tc200_l599": (200, 200 * 2 + 199, 320, 1),
    "tc512_l521": (512, 512 + 9, 64, 2),
    "tc520_l4197": (520, 520 * 8 + 37, 72, 1),
}
CASES = {}
for _n, _s in _SHAPES.items():
    CASES[_n + "_f32"] = Case(*_s, F32)
    CASES[_n + "_bf16"] = Case(*_s, BF16)
CASES["nosoftplus_f32"] = Case(72, 72 * 2 + 15, 72, 2, F32, softplus=0, null_bias=True)
CASES["nullparams_bf16"] = Case(64, 64 * 2 + 9, 40, 1, BF16, null_D=True, null_bias=True)
CASES["strided_f32"] = Case(72, 72 * 2 + 15, 72, 2, F32, strided=True)
CASES["strided_bf16"] = Case(72, 72 * 2 + 15, 72, 2, BF16, strided=True)
CASES["one_l37_f32"] = Case(64, 37, 200, 3, F32, null_ws=True)
CASES["one_l343_bf16"] = Case(344, 343, 96, 2, BF16, null_ws=True)


# ------------------------------------------------------------------------------------------------ fp64 side (CPU)
def _draw(B, L, Dx, dtype, softplus, null_D, null_bias, seed):
    """CPU f32 tensors holding values representable in `dtype` (A, D, delta_bias are f32 parameters)."""
    g = torch.Generator().manual_seed(seed)
    q = lambda t: t.to(dtype).float()  # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    u = q(rn(B, L, Dx))
    delta = q(rn(B, L, Dx) * 0.5 - 1.0) if softplus else q(rn(B, L, Dx).abs() * 0.2 + 0.01)
    A = -torch.exp(rn(Dx, N) * 0.3)
    Bm, Cm = q(rn(B, L, N)), q(rn(B, L, N))
    D, bias = rn(Dx), rn(Dx) * 0.1
    dy = q(rn(B, L, Dx))
    return dict(u=u, delta=delta, A=A, Bm=Bm, Cm=Cm, D=None if null_D else D, bias=None if null_bias else bias, dy=dy)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = CASES[name]
    return _draw(c.B, c.L, c.Dx, c.dtype, c.softplus, c.null_D, c.null_bias, 7000 + list(CASES).index(name))


def _chunk_sums(x, Tc):
    """(B, L, ...) -> (B, nch, ...): sums over the chunks of Tc steps."""
    return np.add.reduceat(x, np.arange(0, x.shape[1], Tc), axis=1)


def _reference(inp, Tc, softplus):
    """The scan, its seven gradients and the stage quantities of the module docstring: fp64, one step at a time."""
    f = lambda t: None if t is None else t.double().numpy()  # noqa: E731
    u, delta, A, Bm, Cm, D, bias, dy = (f(inp[k]) for k in ("u", "delta", "A", "Bm", "Cm", "D", "bias", "dy"))
    B, L, Dx = u.shape
    nch = -(-L // Tc)
    pre = delta if bias is None else delta + bias
    dt = np.where(pre > 20.0, pre, np.log1p(np.exp(np.minimum(pre, 20.0)))) if softplus else pre
    at = np.exp(dt[..., None] * A)                                  # (B, L, Dx, N)
    inj = (dt * u)[..., None] * Bm[:, :, None, :]
    xs = np.zeros((B, L + 1, Dx, N))                                # xs[:, t]: the state before step t
    xend = np.zeros((B, nch, Dx, N))
    xl = np.zeros((B, Dx, N))
    for t in range(L):
        if t % Tc == 0:
            xl = np.zeros((B, Dx, N))
        xs[:, t + 1] = at[:, t] * xs[:, t] + inj[:, t]
        xl = at[:, t] * xl + inj[:, t]
        if (t + 1) % Tc == 0 or t == L - 1:
            xend[:, t // Tc] = xl
    y = np.einsum("bldn,bln->bld", xs[:, 1:], Cm)
    if D is not None:
        y = y + D * u
    lam = np.zeros((B, L, Dx, N))
    gl, gin = np.zeros((B, nch, Dx, N)), np.zeros((B, nch, Dx, N))
    h = np.zeros((B, Dx, N))
    hl = np.zeros((B, Dx, N))
    for t in range(L - 1, -1, -1):
        if (t + 1) % Tc == 0 or t == L - 1:                         # the chunk's last step
            gin[:, t // Tc] = h
            hl = np.zeros((B, Dx, N))
        cg = Cm[:, t, None, :] * dy[:, t, :, None]
        lam[:, t] = cg + h
        h = at[:, t] * lam[:, t]
        hl = at[:, t] * (cg + hl)
        if t % Tc == 0:
            gl[:, t // Tc] = hl
    sgB = np.einsum("bldn,bln->bld", lam, Bm)
    gax = lam * at * xs[:, :L]                                      # lambda_t a_t x_{t-1}
    du = dt * sgB + (0.0 if D is None else D * dy)
    ddt = u * sgB + (gax * A).sum(-1)
    ddelta = ddt * np.where(pre > 20.0, 1.0, 1.0 / (1.0 + np.exp(-pre))) if softplus else ddt
    dB = np.einsum("bldn,bld->bln", lam, dt * u)
    dC = np.einsum("bldn,bld->bln", xs[:, 1:], dy)
    dA_part = _chunk_sums(gax * dt[..., None], Tc)
    dD_part = _chunk_sums(dy * u, Tc)
    db_part = _chunk_sums(ddelta, Tc)
    return dict(y=y, sdt=_chunk_sums(dt, Tc), xend=xend, xinit=xs[:, 0:L:Tc].copy(), ckpt=xs[:, 0:L:CKPT].copy(),
                gl=gl, gin=gin, du=du, ddelta=ddelta, dBC=np.concatenate([dB, dC], -1), dA_part=dA_part,
                dD_part=dD_part, db_part=db_part, dA=dA_part.sum((0, 1)), dD=dD_part.sum((0, 1)),
                ddb=db_part.sum((0, 1)), A=A)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Computed once per case, shared by the tests, never modified."""
    c = CASES[name]
    return _reference(_inputs(name), c.Tc, c.softplus)


@pytest.mark.parametrize("softplus,null_D,null_bias", [(1, False, False), (0, False, True), (1, True, True)])
def test_reference_is_pinned_by_the_oracle(softplus, null_D, null_bias):
    """The test's own fp64 loop against oracle.selective_scan with autograd in fp64 (y and the seven gradients), and
    the stage quantities against the carry recurrences they are defined by. CPU only."""
    B, L, Dx, Tc = 2, 21, 5, 8
    inp = _draw(B, L, Dx, F32, softplus, null_D, null_bias, 11)
    ref = _reference(inp, Tc, softplus)
    cm = lambda t: t.double().transpose(1, 2).contiguous().requires_grad_(True)  # noqa: E731
    u, delta, Bm, Cm = (cm(inp[k]) for k in ("u", "delta", "Bm", "Cm"))
    A = inp["A"].double().requires_grad_(True)
    D = None if null_D else inp["D"].double().requires_grad_(True)
    bias = None if null_bias else inp["bias"].double().requires_grad_(True)
    y = oscan.selective_scan(u, delta, A, Bm, Cm, D, delta_bias=bias, delta_softplus=bool(softplus))
    (y * inp["dy"].double().transpose(1, 2)).sum().backward()
    close = lambda a, b: np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-11, atol=1e-12)  # noqa: E731
    close(ref["y"], y.transpose(1, 2))
    close(ref["du"], u.grad.transpose(1, 2))
    close(ref["ddelta"], delta.grad.transpose(1, 2))
    close(ref["dBC"][..., :N], Bm.grad.transpose(1, 2))
    close(ref["dBC"][..., N:], Cm.grad.transpose(1, 2))
    close(ref["dA"], A.grad)
    if not null_D:
        close(ref["dD"], D.grad)
    if not null_bias:
        close(ref["ddb"], bias.grad)
    nch = ref["xend"].shape[1]
    decay = np.exp(ref["A"][None, None] * ref["sdt"][..., None])     # (B, nch, Dx, N)
    assert not ref["xinit"][:, 0].any() and not ref["gin"][:, nch - 1].any() and not ref["ckpt"][:, 0].any()
    for c in range(nch - 1):
        np.testing.assert_allclose(ref["xinit"][:, c + 1], decay[:, c] * ref["xinit"][:, c] + ref["xend"][:, c],
                                   rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(ref["gin"][:, c], ref["gl"][:, c + 1] + decay[:, c + 1] * ref["gin"][:, c + 1],
                                   rtol=1e-11, atol=1e-13)


# ------------------------------------------------------------------------------------------------ device side
class _Buf:
    """A view of `shape` (unit last stride, row stride `row` >= shape[-1]) inside a flat buffer: sentinel guard bands
    on both sides and in the pad columns, the view itself pre-filled with `fill`."""

    def __init__(self, shape, dtype, fill, row=None):
        row = row or shape[-1]
        n = math.prod(shape[:-1]) * row
        self.flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.flat[GUARD:GUARD + n].view(*shape[:-1], row)[..., :shape[-1]]
        self.view.fill_(fill)
        inside = torch.zeros(n + 2 * GUARD, dtype=torch.bool, device="cuda")
        inside[GUARD:GUARD + n].view(*shape[:-1], row)[..., :shape[-1]] = True
        self.outside = ~inside
        self.before = self.flat.clone()

    @staticmethod
    def _bits(t):
        return t.view(torch.int16 if t.dtype == BF16 else torch.int32)

    def outside_intact(self):
        return torch.equal(self._bits(self.flat)[self.outside], self._bits(self.before)[self.outside])

    def unchanged(self):
        return torch.equal(self._bits(self.flat), self._bits(self.before))

    def ptr(self):
        return self.view.data_ptr()


def _place(t, dtype, row=None):
    """A CPU (B, L, C) tensor on the device as the first C columns of NaN-filled rows of `row` elements."""
    B, L, C = t.shape
    full = torch.full((B, L, row or C), float("nan"), dtype=dtype, device="cuda")
    full[..., :C] = t.to("cuda", dtype)
    return full[..., :C]


def _bt(t):
    return [t.stride(0), t.stride(1)]


def _expected_plain(Dx, Tc):
    nwv = max(1, min(1 if Tc >= 512 else 4, -(-Dx // 64)))
    return int(-(-Dx // (nwv * 64)) == 1)


def _launch(c, inp, fill, bad=None):
    """Both entry points on fresh guarded buffers. `bad` (host-check tests) replaces one argument by an invalid one;
    the calls are then expected to raise before anything is launched."""
    from long_context_biomedical_imaging_amd import _lib
    bad = bad or {}
    B, L, Dx = inp["u"].shape
    dt, Tc = c.dtype, c.Tc
    nch, nck = -(-L // bad.get("alloc_tc", Tc)), -(-L // CKPT)
    row = Dx + PAD if c.strided else Dx
    u, delta, dy = (_place(inp[k], dt, row) for k in ("u", "delta", "dy"))
    r0 = (R if c.strided else 0) + bad.get("b_offset", 0)
    bc = torch.full((B, L, r0 + 2 * N), float("nan"), dtype=dt, device="cuda")
    bc[..., r0:r0 + N] = inp["Bm"].to("cuda", dt)
    bc[..., r0 + N:] = inp["Cm"].to("cuda", dt)
    Bv, Cv = bc[..., r0:r0 + N], bc[..., r0 + N:]
    A = inp["A"].cuda().contiguous()
    D = None if inp["D"] is None else inp["D"].cuda()
    bias = None if inp["bias"] is None else inp["bias"].cuda()
    plain = _lib.load().lci_selective_scan_bwd_plain_dbc(L, Dx, Tc)
    bufs = dict(
        y=_Buf((B, L, Dx), dt, fill, 2 * Dx if c.strided else Dx),
        ckpt=_Buf((B, nck, Dx, N), dt, fill),
        du=_Buf((B, L, Dx), dt, fill, row), ddelta=_Buf((B, L, Dx), dt, fill, row),
        dBC=_Buf((B, L, 2 * N), F32, fill if plain or bad else 0.0),
        dA=_Buf((Dx, N), F32, fill if bad else 0.0), dD=_Buf((Dx,), F32, fill if bad else 0.0),
        ddb=_Buf((Dx,), F32, fill if bad else 0.0),
        gl=_Buf((B, nch, Dx, N), F32, fill), gin=_Buf((B, nch, Dx, N), F32, fill))
    if not c.null_ws:
        bufs.update(xend=_Buf((B, nch, Dx, N), F32, fill), xinit=_Buf((B, nch, Dx, N), F32, fill),
                    sdt=_Buf((B, nch, Dx), F32, fill))
    p = lambda k: bufs[k].ptr() if k in bufs else None  # noqa: E731
    sdt_ptr = None if bad.get("null_sdt") else p("sdt")
    y, du, dd = bufs["y"].view, bufs["du"].view, bufs["ddelta"].view
    dims = (B, L, bad.get("Dx", Dx), bad.get("N", N), bad.get("chunk", Tc), c.softplus)
    code, stream = _lib.DTYPE[dt], _lib.stream_of(u)
    fs = _lib.c_array(ctypes.c_longlong, [*_bt(u), *_bt(delta), *_bt(Bv), *_bt(Cv), *_bt(y), 0, 0, 0, 0, 0, 0])
    bs = _lib.c_array(ctypes.c_longlong, [*_bt(u), *_bt(delta), *_bt(Bv), *_bt(Cv), 0, 0, *_bt(dy), *_bt(du), *_bt(dd)])
    fwd = lambda: _lib.call(  # noqa: E731
        "lci_selective_scan_fwd", code, u.data_ptr(), delta.data_ptr(), A.data_ptr(), Bv.data_ptr(), Cv.data_ptr(),
        _lib.ptr(D), _lib.ptr(bias), p("y"), fs, *dims, p("xend"), p("xinit"), sdt_ptr, p("ckpt"), stream)
    bwd = lambda: _lib.call(  # noqa: E731
        "lci_selective_scan_bwd", code, u.data_ptr(), delta.data_ptr(), A.data_ptr(), Bv.data_ptr(), Cv.data_ptr(),
        _lib.ptr(D), _lib.ptr(bias), dy.data_ptr(), p("du"), p("ddelta"), p("dBC"), p("dA"), p("dD"), p("ddb"), bs,
        *dims, sdt_ptr, p("ckpt"), p("gl"), p("gin"), stream)
    if bad:
        for call in (fwd, bwd):
            with pytest.raises(_lib.LciError):
                call()
        torch.cuda.synchronize()
        return {k: b.unchanged() for k, b in bufs.items()}
    fwd()
    bwd()
    torch.cuda.synchronize()
    out = {k: b.view.detach().cpu().clone() for k, b in bufs.items()}
    out["_intact"] = {k: b.outside_intact() for k, b in bufs.items()}
    out["_plain"] = plain
    return out


@functools.lru_cache(maxsize=None)
def _run(name, fill="nan", sample=None):
    c, inp = CASES[name], _inputs(name)
    if sample is not None:
        inp = {k: v[sample:sample + 1] if k in ("u", "delta", "Bm", "Cm", "dy") else v for k, v in inp.items()}
    return _launch(c, inp, FILLS[fill])


# ------------------------------------------------------------------------------------------------ metrics
class _Report:
    def __init__(self, name):
        self.name, self.rows, self.fails = name, [], []

    def _group(self, what, x, ref, keep, bound):
        """Largest rel-L2 over the groups indexed by the axes `keep` (norms over every other axis). A group whose
        reference is identically zero must be exactly zero."""
        red = tuple(i for i in range(ref.ndim) if i not in keep)
        num = np.sqrt(((x - ref) ** 2).sum(axis=red)) if red else np.abs(x - ref)
        den = np.sqrt((ref ** 2).sum(axis=red)) if red else np.abs(ref)
        num, den = np.atleast_1d(num), np.atleast_1d(den)
        zero = den == 0
        if (zero & ~(num == 0)).any():      # (a NaN fails here too)
            self.fails.append(f"{what}: nonzero where the reference is identically zero")
        rel = float((num[~zero] / den[~zero]).max()) if (~zero).any() else 0.0
        if not rel <= bound:
            self.fails.append(f"{what}: rel-L2 {rel:.3e} > {bound:.1e}")
        return rel

    def check(self, q, x, ref, bound, group_axis=None, windows=None):
        x = x.double().numpy() if isinstance(x, torch.Tensor) else x
        whole = self._group(f"{q} whole", x, ref, (), bound)
        sample = self._group(f"{q} per sample", x, ref, (0,), bound) if group_axis is not None or windows else whole
        win = 0.0
        if group_axis is not None:
            win = self._group(f"{q} per chunk/checkpoint", x, ref, (group_axis,), bound)
        for lo, hi in windows or ():
            win = max(win, self._group(f"{q} tokens [{lo}, {hi})", x[:, lo:hi], ref[:, lo:hi], (), bound))
        self.rows.append((q, whole, sample, win, bound))

    def elementwise(self, q, x, ref):
        x = x.double().numpy()
        allowed = U_BF16 * np.abs(ref) + 1e-4 * np.abs(ref).max()
        err = np.abs(x - ref)
        with np.errstate(divide="ignore", invalid="ignore"):    # no allowance (an all-zero reference): exact
            worst = float(np.where(allowed > 0, err / allowed, np.where(err == 0, 0.0, np.inf)).max())
        if not worst <= 1.0:
            self.fails.append(f"{q}: per-element error {worst:.3f} x the allowance")
        self.rows.append((q + "_elem", worst, worst, worst, 1.0))

    def finish(self):
        print(f"\n{self.name}")
        for q, whole, sample, win, bound in self.rows:
            print(f"  {q:<22} whole {whole:.2e}  sample {sample:.2e}  window {win:.2e}  bound {bound:.1e}")
        print("TABLE " + self.name.ljust(20) + " ".join(f"{q}={max(w, s, v):.1e}" for q, w, s, v, _ in self.rows))
        assert not self.fails, "\n".join(self.fails)


def _windows(c):
    """Token windows where chunked code goes wrong: 8 tokens either side of every chunk boundary, the first and last
    8 tokens, the last sub-block."""
    w = {(0, min(8, c.L)), (max(0, c.L - 8), c.L), (CKPT * ((c.L - 1) // CKPT), c.L)}
    for k in range(1, c.nch):
        w.add((max(0, k * c.Tc - 8), min(c.L, k * c.Tc + 8)))
    return sorted(w)


# ------------------------------------------------------------------------------------------------ tests
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_scan_stages_vs_fp64(name):
    """Every output and workspace of one forward + backward against the fp64 loop, whole / per sample / per window,
    with the pre-fill, guard-band and dBC zero-fill checks of the module docstring."""
    c, ref, out = CASES[name], _ref(name), _run(name)
    bf = c.dtype == BF16
    fwd_b, io_b, grad_b = 1e-4, (5e-3 if bf else 1e-4), (5e-3 if bf else 2e-4)
    rep, win = _Report(name), _windows(c)
    assert out["_plain"] == _expected_plain(c.Dx, c.Tc), "lci_selective_scan_bwd_plain_dbc departs from its rule"
    for k, ok in out["_intact"].items():
        if not ok:
            rep.fails.append(f"{k}: guard band or pad column written")
    finite = [k for k in BITWISE if k in out] + ["dBC", "dA", "dD", "ddb"]
    for k in finite:
        if not torch.isfinite(out[k]).all():
            rep.fails.append(f"{k}: non-finite entries left")
    rep.check("y", out["y"], ref["y"], io_b, windows=win)
    if bf:
        rep.elementwise("y", out["y"], ref["y"])
    if not c.null_ws:
        rep.check("sdt", out["sdt"], ref["sdt"], fwd_b, group_axis=1)
        rep.check("xend", out["xend"], ref["xend"], fwd_b, group_axis=1)
        rep.check("xinit", out["xinit"], ref["xinit"], fwd_b, group_axis=1)
    rep.check("ckpt", out["ckpt"], ref["ckpt"], io_b, group_axis=1)
    if bf:
        rep.elementwise("ckpt", out["ckpt"], ref["ckpt"])
    rep.check("du", out["du"], ref["du"], grad_b, windows=win)
    rep.check("ddelta", out["ddelta"], ref["ddelta"], grad_b, windows=win)
    rep.check("dBC", out["dBC"], ref["dBC"], grad_b, windows=win)
    rep.check("dA", out["dA"], ref["dA"], grad_b)
    rep.check("dD", out["dD"], ref["dD"], grad_b)
    rep.check("ddb", out["ddb"], ref["ddb"], grad_b)
    if c.partials:
        gl, gin = out["gl"], out["gin"]
        if not (torch.isfinite(gin).all() and torch.isfinite(gl[..., :2]).all()):
            rep.fails.append("parameter partials: non-finite entries left")
        rep.check("dA_part", gin, ref["dA_part"], grad_b, group_axis=1)
        rep.check("dD_part", gl[..., 0], ref["dD_part"], grad_b, group_axis=1)
        rep.check("db_part", gl[..., 1], ref["db_part"], grad_b, group_axis=1)
    else:
        rep.check("gl", out["gl"], ref["gl"], grad_b, group_axis=1)
        rep.check("gin", out["gin"], ref["gin"], grad_b, group_axis=1)
    rep.finish()


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_scan_deterministic_and_slice_invariant(name):
    """Two runs over differently pre-filled buffers, and the last sample repacked as a B = 1 problem."""
    c, a, b = CASES[name], _run(name), _run(name, "three")
    assert all(b["_intact"].values())
    for k in BITWISE:
        if k in a:
            assert torch.equal(a[k], b[k]), f"{k}: two runs differ"
    for k in ATOMIC:
        err = (a[k] - b[k]).abs().max().item()
        assert err <= 1e-4 * b[k].abs().max().item() + 1e-6, (k, err)
    if c.B > 1:
        s = _run(name, "nan", c.B - 1)
        for k in BITWISE:
            if k in a:
                assert torch.equal(s[k][0], a[k][c.B - 1]), f"{k}: the B = 1 repack of a sample differs from its slice"


@gpu
@pytest.mark.parametrize("what,bad", [("N4", dict(N=4)), ("chunk12", dict(chunk=12)), ("Dx1025", dict(Dx=1025)),
                                      ("misaligned_B", dict(b_offset=4)), ("null_sdt", dict(null_sdt=True))])
def test_scan_host_checks(what, bad):
    """Each invalid call raises LciError from both entry points and leaves every NaN-pre-filled output untouched.
    L = 80 in two chunks of 64 / 16 steps; every buffer is sized for the extents passed (the workspaces for chunks of
    8 steps, more than any chunk length used here needs)."""
    c = Case(64, 80, bad.get("Dx", 24), 1, BF16)
    inp = _draw(c.B, c.L, c.Dx, c.dtype, 1, False, False, 99)
    unchanged = _launch(c, inp, float("nan"), dict(bad, alloc_tc=CKPT))
    assert all(unchanged.values()), [k for k, v in unchanged.items() if not v]
