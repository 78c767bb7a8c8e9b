"""GPU: the deterministic mode (kernels.deterministic_mode, the *_det entry points of include/lci.h).

Every case computes its gradients three times on identical inputs, with every output and workspace buffer pre-filled
differently per run (NaN, 3.0, zeros: the convention of test_scan_kernel_gpu.py), and requires
  1. all three runs to agree on the raw bits of every returned gradient (torch.equal on integer views, so a NaN cannot
     compare equal by accident), every value finite;
  2. the gradients to agree with an fp64 reference, computed from the rounded inputs the kernel saw, within the bound
     the project already uses for that quantity (rel-L2 over the whole tensor):
       scan                  2e-4 in f32, 5e-3 in bf16 (tests/test_scan_kernel_gpu.py:56-58, derived there)
       Hyena short conv      dz 1e-5, dw / db 1e-4 in f32; 1e-2 for all three in bf16 (tests/test_hyena_gpu.py:197-206)
       long-conv du, dD      1e-4 (tests/test_hyena_gpu.py:170-172); the op is f32 only, its "bf16" form feeds it
                             bf16-representable values
       patch embedding       dw, db 1e-4, dpos 1e-5 (tests/test_modules_gpu.py:53-56); the kernel accumulates in f32
                             from the rounded inputs, so the same bounds serve bf16 I/O

A. Selective scan through lci_selective_scan_fwd + lci_selective_scan_bwd_det with an explicit chunk Tc, against the
   fp64 step loop of test_scan_kernel_gpu.py (copied here). (Tc, L, Dx, B) and the structure each case reaches:
     A1  64, 133, 320, 2   4-wave workgroups (per-wave LDS slots added in wave order), two channel groups (dBC slabs
                           + ordered sum), parameter partials over 6 rows
     A2  72, 303, 264, 2   mid-chunk flush; a second channel group with three padded waves
     A3  512, 521, 72, 2   Tc >= 512 (the default mode's atomics for dA / dD / d(delta_bias)), two one-wave workgroups
     A4  8, 533, 24, 1     67 partial rows through the ordered sum (4 row slices)
     A5  64, 37, 200, 3    one chunk, sdt null
     A6  A1's inputs through kernels.selective_scan_cl under kernels.deterministic_mode(), joint B|C and separate B, C
   The workspace query is asserted against its rule: one (B, L, 16) f32 slab per channel group when there are several.
B. lci_hyena_pre_bwd_det (BB 2, D = 2 heads x 40: a partly filled second channel block; K 3 and 5, with and without
   bias) against an fp64 torch composite. hg_v3_ok takes bf16 with hd % 8 == 0, D % 8 == 0, L % 4 == 0 and 16-byte
   pointers: B1 = bf16, L 300 runs the persistent bwd3 kernel (five 64-token tiles, the last ragged); B2 = f32, L 300
   and bf16, L 302 run the bwd2 fallback (three 128-token tiles, the last ragged); the bwd3 kernel has no f32 form.
   B3: lci_fftconv_bwd_det without dk, (R, C, L) = (3, 5, 16384 + 37) (two splits, scalar loads) and (3, 5, 32768)
   (16-byte loads), against an fp64 FFT correlation / dot product.
C. lci_patch_embed_bwd_det against fp64 conv autograd. C1: B 3, C 1, 36 x 36, patch 2, D 8, channels-last with pos
   (L 324: two workgroups per sample); C2: B 2, C 2, (6, 10, 10), patch 2, D 6, channels-first, with and without
   bias; C3: C1's image at B 600, where a sample's two tiles share one workgroup (the bounded partial buffer) and 600
   rows go through the ordered sum's 16 row slices.
D. The default mode is untouched: for A1, B1 and C1 its gradients meet the same fp64 bounds (not bitwise equal to the
   deterministic ones: the two modes add in different orders).
E. MambaVisionMixer and HyenaOperator (the sizes of the golden module cases of tests/test_mamba_gpu.py and
   tests/test_hyena_gpu.py) built twice from one seed, forward + backward under bf16 autocast and
   kernels.deterministic_mode(): every parameter gradient and the input gradient agree bit for bit.
H. Two TrainStep.step calls with --deterministic --use_amp on one synthetic batch, the model built twice from one
   seed, torch.use_deterministic_algorithms(True, warn_only=True) set inside the test and restored: every parameter
   agrees bit for bit. Swin-tiny patch 2 + UperNet3D on a 32^3 volume with Mamba in 4^3 windows and with Hyena in 8^3
   windows (bench.py's recipe workloads, smaller), and ViT-small patch 2 + ViTUNETR with the Mamba mixer on 16^3
   (tests/test_ddp_model_gpu.py's vit_mamba_unetr).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from golden_util import Golden, cotangents

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF16]
N = 8
CKPT = 8
FILLS = (float("nan"), 3.0, 0.0)


def _ids(v):
    return {F32: "f32", BF16: "bf16"}.get(v, None) if isinstance(v, torch.dtype) else None


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _rel(x, ref):
    x = np.asarray(x.detach().double().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    ref = np.asarray(ref.detach().double().cpu() if isinstance(ref, torch.Tensor) else ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return float(np.sqrt(((x - ref) ** 2).sum()) / max(np.sqrt((ref ** 2).sum()), 1e-300))


def _check(name, runs, ref, bounds):
    """runs: one {quantity: tensor} per pre-fill; ref: {quantity: fp64 array}; bounds: {quantity: rel-L2 bound}."""
    fails = []
    for q, bound in bounds.items():
        for i, r in enumerate(runs):
            if not torch.isfinite(r[q].float()).all():
                fails.append(f"{q}: run {i} left non-finite values")
            if i and not torch.equal(_bits(r[q]), _bits(runs[0][q])):
                fails.append(f"{q}: run {i} differs from run 0 in its bits")
        e = _rel(runs[0][q], ref[q])
        print(f"{name} {q}: rel-L2 {e:.2e} (bound {bound:.0e})")
        if not e <= bound:
            fails.append(f"{q}: rel-L2 {e:.3e} > {bound:.1e}")
    assert not fails, f"{name}: " + "; ".join(fails)


def _full(fill, *shape, dtype=F32):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def _lib():
    from long_context_biomedical_imaging_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ A: selective scan
SCAN = {"A1": (64, 133, 320, 2), "A2": (72, 303, 264, 2), "A3": (512, 521, 72, 2), "A4": (8, 533, 24, 1),
        "A5": (64, 37, 200, 3)}
SCAN_Q = ("du", "ddelta", "dBC", "dA", "dD", "ddb")


@functools.lru_cache(maxsize=None)
def _scan_inputs(case, dtype):
    """CPU f32 tensors holding values representable in `dtype` (A, D, delta_bias are f32 parameters)."""
    Tc, L, Dx, B = SCAN[case]
    g = torch.Generator().manual_seed(9100 + list(SCAN).index(case))
    q = lambda t: t.to(dtype).float()  # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    u = q(rn(B, L, Dx))
    delta = q(rn(B, L, Dx) * 0.5 - 1.0)
    A = -torch.exp(rn(Dx, N) * 0.3)
    Bm, Cm = q(rn(B, L, N)), q(rn(B, L, N))
    D, bias = rn(Dx), rn(Dx) * 0.1
    dy = q(rn(B, L, Dx))
    return dict(u=u, delta=delta, A=A, Bm=Bm, Cm=Cm, D=D, bias=bias, dy=dy)


@functools.lru_cache(maxsize=None)
def _scan_ref(case, dtype):
    """The seven gradients of the scan in fp64, one step at a time (the loop of test_scan_kernel_gpu.py::_reference,
    softplus on, D and delta_bias given). Computed once per case, never modified."""
    inp = _scan_inputs(case, dtype)
    f = lambda t: t.double().numpy()  # noqa: E731
    u, delta, A, Bm, Cm, D, bias, dy = (f(inp[k]) for k in ("u", "delta", "A", "Bm", "Cm", "D", "bias", "dy"))
    B, L, Dx = u.shape
    pre = delta + bias
    dt = np.where(pre > 20.0, pre, np.log1p(np.exp(np.minimum(pre, 20.0))))
    at = np.exp(dt[..., None] * A)                                  # (B, L, Dx, N)
    inj = (dt * u)[..., None] * Bm[:, :, None, :]
    xs = np.zeros((B, L + 1, Dx, N))                                # xs[:, t]: the state before step t
    for t in range(L):
        xs[:, t + 1] = at[:, t] * xs[:, t] + inj[:, t]
    lam = np.zeros((B, L, Dx, N))
    h = np.zeros((B, Dx, N))
    for t in range(L - 1, -1, -1):
        lam[:, t] = Cm[:, t, None, :] * dy[:, t, :, None] + h
        h = at[:, t] * lam[:, t]
    sgB = np.einsum("bldn,bln->bld", lam, Bm)
    gax = lam * at * xs[:, :L]                                      # lambda_t a_t x_{t-1}
    du = dt * sgB + D * dy
    ddt = u * sgB + (gax * A).sum(-1)
    ddelta = ddt * np.where(pre > 20.0, 1.0, 1.0 / (1.0 + np.exp(-pre)))
    dB = np.einsum("bldn,bld->bln", lam, dt * u)
    dC = np.einsum("bldn,bld->bln", xs[:, 1:], dy)
    return dict(du=du, ddelta=ddelta, dBC=np.concatenate([dB, dC], -1), dA=(gax * dt[..., None]).sum((0, 1)),
                dD=(dy * u).sum((0, 1)), ddb=ddelta.sum((0, 1)))


def _bt(t):
    return [t.stride(0), t.stride(1)]


def _scan_groups(Tc, Dx):
    nwv = max(1, min(1 if Tc >= 512 else 4, -(-Dx // 64)))
    return -(-Dx // (nwv * 64))


def _scan_launch(case, dtype, fill, det=True):
    """lci_selective_scan_fwd, then the deterministic (or the default) backward entry point, on buffers pre-filled
    with `fill` wherever the entry point's contract allows it."""
    lib = _lib()
    Tc, L, Dx, B = SCAN[case]
    inp = _scan_inputs(case, dtype)
    one = case == "A5"
    nch, nck = -(-L // Tc), -(-L // CKPT)
    u, delta, dy = (inp[k].to("cuda", dtype) for k in ("u", "delta", "dy"))
    bc = torch.cat([inp["Bm"], inp["Cm"]], -1).to("cuda", dtype)
    Bv, Cv = bc[..., :N], bc[..., N:]
    A, D, bias = inp["A"].cuda().contiguous(), inp["D"].cuda(), inp["bias"].cuda()
    y, ckpt = _full(fill, B, L, Dx, dtype=dtype), _full(fill, B, nck, Dx, N, dtype=dtype)
    xend = xinit = sdt = None
    if not one:
        xend, xinit, sdt = _full(fill, B, nch, Dx, N), _full(fill, B, nch, Dx, N), _full(fill, B, nch, Dx)
    code, stream = lib.DTYPE[dtype], lib.stream_of(u)
    dims = (B, L, Dx, N, Tc, 1)
    fs = lib.c_array(ctypes.c_longlong, [*_bt(u), *_bt(delta), *_bt(Bv), *_bt(Cv), *_bt(y), 0, 0, 0, 0, 0, 0])
    lib.call("lci_selective_scan_fwd", code, u.data_ptr(), delta.data_ptr(), A.data_ptr(), Bv.data_ptr(),
             Cv.data_ptr(), D.data_ptr(), bias.data_ptr(), y.data_ptr(), fs, *dims, lib.ptr(xend), lib.ptr(xinit),
             lib.ptr(sdt), ckpt.data_ptr(), stream)
    du, dd = _full(fill, B, L, Dx, dtype=dtype), _full(fill, B, L, Dx, dtype=dtype)
    gl, gin = _full(fill, B, nch, Dx, N), _full(fill, B, nch, Dx, N)
    bs = lib.c_array(ctypes.c_longlong, [*_bt(u), *_bt(delta), *_bt(Bv), *_bt(Cv), 0, 0, *_bt(dy), *_bt(du), *_bt(dd)])
    if det:
        dBC, dA, dD, ddb = _full(fill, B, L, 2 * N), _full(fill, Dx, N), _full(fill, Dx), _full(fill, Dx)
        nbytes = lib.load().lci_selective_scan_bwd_det_ws_bytes(B, L, Dx, Tc)
        ng = _scan_groups(Tc, Dx)
        assert nbytes == (ng * B * L * 2 * N * 4 if ng > 1 else 0), (nbytes, ng)
        ws = _full(fill, max(1, nbytes // 4))
        tail, name = (ws.data_ptr(),), "lci_selective_scan_bwd_det"
    else:   # the default contract: accumulated outputs are zeroed by the caller (dBC only where it is not plain)
        plain = lib.load().lci_selective_scan_bwd_plain_dbc(L, Dx, Tc)
        dBC = _full(fill if plain else 0.0, B, L, 2 * N)
        dA, dD, ddb = _full(0.0, Dx, N), _full(0.0, Dx), _full(0.0, Dx)
        tail, name = (), "lci_selective_scan_bwd"
    lib.call(name, code, u.data_ptr(), delta.data_ptr(), A.data_ptr(), Bv.data_ptr(), Cv.data_ptr(), D.data_ptr(),
             bias.data_ptr(), dy.data_ptr(), du.data_ptr(), dd.data_ptr(), dBC.data_ptr(), dA.data_ptr(), dD.data_ptr(),
             ddb.data_ptr(), bs, *dims, lib.ptr(sdt), ckpt.data_ptr(), gl.data_ptr(), gin.data_ptr(), *tail, stream)
    torch.cuda.synchronize()
    return dict(du=du, ddelta=dd, dBC=dBC, dA=dA, dD=dD, ddb=ddb)


def _scan_bounds(dtype):
    return dict.fromkeys(SCAN_Q, 5e-3 if dtype == BF16 else 2e-4)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", list(SCAN))
def test_scan_bwd_det(case, dtype):
    runs = [_scan_launch(case, dtype, fill) for fill in FILLS]
    _check(f"{case}_{_ids(dtype)}", runs, _scan_ref(case, dtype), _scan_bounds(dtype))


def _pollute(fill):
    """Leave freed blocks holding `fill` in the caching allocator, so the torch.empty buffers of an op that allocates
    its own outputs and workspaces start from different contents in each run."""
    junk = [torch.full((1 << k,), fill, device="cuda") for k in range(8, 23)]
    del junk


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("joint", [True, False], ids=["joint_bc", "separate_bc"])
def test_scan_autograd_op_det(joint, dtype):
    """A6: kernels.selective_scan_cl under kernels.deterministic_mode() on A1's inputs."""
    from long_context_biomedical_imaging_amd import kernels
    Tc, L, Dx, B = SCAN["A1"]
    assert kernels._scan_chunk(L, B, Dx) == Tc
    inp = _scan_inputs("A1", dtype)
    ref = _scan_ref("A1", dtype)
    runs = []
    for fill in FILLS:
        _pollute(fill)
        u, delta, dy = (inp[k].to("cuda", dtype) for k in ("u", "delta", "dy"))
        u.requires_grad_(True), delta.requires_grad_(True)
        A, D, bias = (inp[k].cuda().requires_grad_(True) for k in ("A", "D", "bias"))
        bc = torch.cat([inp["Bm"], inp["Cm"]], -1).to("cuda", dtype)
        if joint:
            Bm, Cm = bc.requires_grad_(True), None
        else:
            Bm, Cm = bc[..., :N].contiguous().requires_grad_(True), bc[..., N:].contiguous().requires_grad_(True)
        yz = torch.zeros(B, L, 2 * Dx, device="cuda", dtype=dtype)
        with kernels.deterministic_mode():
            out = kernels.selective_scan_cl(u, delta, A, Bm, Cm, D, bias, yz)
        cot = torch.zeros_like(out)
        cot[..., :Dx] = dy
        out.backward(cot)              # outside the block: the backward follows the mode its forward saw
        torch.cuda.synchronize()
        dBC = Bm.grad if joint else torch.cat([Bm.grad, Cm.grad], -1)
        runs.append(dict(du=u.grad, ddelta=delta.grad, dBC=dBC, dA=A.grad, dD=D.grad, ddb=bias.grad))
    _check(f"A6_{'joint' if joint else 'separate'}_{_ids(dtype)}", runs, ref, _scan_bounds(dtype))


# ------------------------------------------------------------------------------------------------ B: Hyena
HY_BB, HY_H, HY_HD = 2, 2, 40
HYENA = {  # name: (dtype, L, K, bias)
    "B1_bwd3_k3_bias": (BF16, 300, 3, True), "B1_bwd3_k5_nobias": (BF16, 300, 5, False),
    "B2_bwd2_f32_k3_nobias": (F32, 300, 3, False), "B2_bwd2_f32_k5_bias": (F32, 300, 5, True),
    "B2_bwd2_bf16_k5_bias": (BF16, 302, 5, True),
}


@functools.lru_cache(maxsize=None)
def _hyena_case(name):
    """Inputs (rounded to the I/O dtype where the kernel reads that dtype) and the fp64 gradients of the short conv +
    pre-gate (hyena.py:317-333 as restated in tests/test_hyena_gpu.py): causal depthwise conv, per head x1 / x2 / v,
    vg = v x1; cotangents dvg of vg and gx2 of x2."""
    dtype, L, K, has_b = HYENA[name]
    BB, H, hd = HY_BB, HY_H, HY_HD
    D = H * hd
    g = torch.Generator().manual_seed(9200 + list(HYENA).index(name))
    z = torch.randn(BB, L, 3 * D, generator=g).to(dtype).float()
    w = torch.randn(3 * D, K, generator=g) * 0.5
    b = torch.randn(3 * D, generator=g) * 0.1 if has_b else None
    dvg = torch.randn(BB, D, L, generator=g)
    gx2 = torch.randn(BB, L, D, generator=g).to(dtype).float()
    zr, wr = z.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if has_b else None
    conv = torch.nn.functional.conv1d(zr.transpose(1, 2), wr[:, None], br, padding=K - 1, groups=3 * D)[..., :L]
    conv = conv.view(BB, H, 3, hd, L)
    x1, x2, v = (conv[:, :, i].reshape(BB, D, L) for i in range(3))
    ((v * x1 * dvg.double()).sum() + (x2.transpose(1, 2) * gx2.double()).sum()).backward()
    ref = dict(dz=zr.grad.numpy(), dw=wr.grad.numpy())
    if has_b:
        ref["db"] = br.grad.numpy()
    return dict(z=z, w=w, b=b, dvg=dvg, gx2=gx2), ref


def _hyena_launch(name, fill, det=True):
    lib = _lib()
    dtype, L, K, has_b = HYENA[name]
    BB, H, hd = HY_BB, HY_H, HY_HD
    D = H * hd
    inp, _ = _hyena_case(name)
    z, gx2 = inp["z"].to("cuda", dtype), inp["gx2"].to("cuda", dtype)
    w, dvg = inp["w"].cuda().contiguous(), inp["dvg"].cuda()
    b = inp["b"].cuda() if has_b else None
    dz = _full(fill, BB, L, 3 * D, dtype=dtype)
    ofill = fill if det else 0.0      # the default entry point accumulates into zeroed dw / db
    dw = _full(ofill, 3 * D, K)
    db = _full(ofill, 3 * D) if has_b else None
    head = (lib.DTYPE[dtype], z.data_ptr(), w.data_ptr(), lib.ptr(b), dvg.data_ptr(), gx2.data_ptr(), dz.data_ptr(),
            dw.data_ptr(), lib.ptr(db))
    if det:
        nbytes = lib.load().lci_hyena_pre_bwd_det_ws_bytes(BB, L, H, hd, K)
        assert nbytes > 0 and nbytes % (3 * D * (K + 1) * 4) == 0
        ws = _full(fill, nbytes // 4)
        lib.call("lci_hyena_pre_bwd_det", *head, ws.data_ptr(), BB, L, H, hd, K, lib.stream_of(z))
    else:
        lib.call("lci_hyena_pre_bwd", *head, BB, L, H, hd, K, lib.stream_of(z))
    torch.cuda.synchronize()
    out = dict(dz=dz, dw=dw)
    if has_b:
        out["db"] = db
    return out


def _hyena_bounds(name):
    dtype, _, _, has_b = HYENA[name]
    b = dict(dz=1e-5, dw=1e-4) if dtype == F32 else dict(dz=1e-2, dw=1e-2)
    if has_b:
        b["db"] = b["dw"]
    return b


@pytest.mark.parametrize("name", list(HYENA))
def test_hyena_pre_bwd_det(name):
    runs = [_hyena_launch(name, fill) for fill in FILLS]
    _check(name, runs, _hyena_case(name)[1], _hyena_bounds(name))


@functools.lru_cache(maxsize=None)
def _fftconv_case(L, dtype):
    R, C = 3, 5
    g = torch.Generator().manual_seed(9300 + L)
    q = lambda t: t.to(dtype).float()  # noqa: E731
    u, dy = q(torch.randn(R, C, L, generator=g)), q(torch.randn(R, C, L, generator=g))
    k = torch.randn(C, L, generator=g) * torch.exp(-torch.linspace(0, 12, L))[None]
    Dv = torch.randn(C, generator=g)
    n = 2 * L
    cd, ud, kd = dy.double(), u.double(), k.double()
    du = (torch.fft.irfft(torch.fft.rfft(cd.flip(-1), n) * torch.fft.rfft(kd, n), n)[..., :L].flip(-1)
          + cd * Dv.double()[:, None])
    return dict(u=u, dy=dy, k=k, D=Dv), dict(du=du.numpy(), dD=(cd * ud).sum((0, 2)).numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("L", [16384 + 37, 32768], ids=["two_splits_scalar", "vec16"])
def test_fftconv_bwd_dd_without_dk_det(L, dtype):
    """B3: du and the dD of the `dD && !dk` branch, per-(row, split) partials + the ordered sum."""
    from long_context_biomedical_imaging_amd import kernels
    lib = _lib()
    R, C = 3, 5
    inp, ref = _fftconv_case(L, dtype)
    u, dy = inp["u"].cuda(), inp["dy"].cuda()
    K = kernels._spectrum(inp["k"].cuda().contiguous(), inp["D"].cuda())
    n = K.shape[1]
    tw = kernels._twiddles(n, u.device)
    nbytes = lib.load().lci_fftconv_bwd_det_ws_bytes(R, C, L)
    assert nbytes == R * 2 * C * 4
    runs = []
    for fill in FILLS:
        du, dD = _full(fill, R, C, L), _full(fill, C)
        S = _full(fill, C * ((R + 1) // 2), n, 2)
        ws = _full(fill, nbytes // 4)
        lib.call("lci_fftconv_bwd_det", dy.data_ptr(), u.data_ptr(), K.data_ptr(), None, du.data_ptr(), None,
                 dD.data_ptr(), S.data_ptr(), None, None, None, tw.data_ptr(), ws.data_ptr(), R, C, L,
                 lib.stream_of(u))
        torch.cuda.synchronize()
        runs.append(dict(du=du, dD=dD))
    _check(f"B3_L{L}_{_ids(dtype)}", runs, ref, dict(du=1e-4, dD=1e-4))


# ------------------------------------------------------------------------------------------------ C: patch embedding
PATCH = {  # name: (B, C, S, P, D, channels_last, bias)
    "C1_vit_2d": (3, 1, (36, 36), (2, 2), 8, True, True),
    "C2_swin_3d_bias": (2, 2, (6, 10, 10), (2, 2, 2), 6, False, True),
    "C2_swin_3d_nobias": (2, 2, (6, 10, 10), (2, 2, 2), 6, False, False),
    "C3_vit_2d_b600": (600, 1, (36, 36), (2, 2), 8, True, True),
}


@functools.lru_cache(maxsize=None)
def _patch_case(name, dtype):
    B, C, S, P, D, cl, has_b = PATCH[name]
    g = torch.Generator().manual_seed(9400 + list(PATCH).index(name))
    G = [s // p for s, p in zip(S, P)]
    L = int(np.prod(G))
    x = torch.rand(B, C, *S, generator=g).to(dtype).float()
    dy = torch.randn((B, L, D) if cl else (B, D, *G), generator=g).to(dtype).float()
    w = torch.zeros(D, C, *P, dtype=torch.float64, requires_grad=True)      # d/dw, d/db do not depend on w, b
    b = torch.zeros(D, dtype=torch.float64, requires_grad=True) if has_b else None
    conv = torch.nn.functional.conv2d if len(S) == 2 else torch.nn.functional.conv3d
    y = conv(x.double(), w, b, stride=P)                                    # (B, D, *G)
    cot = dy.double().transpose(1, 2).reshape(B, D, *G) if cl else dy.double()
    (y * cot).sum().backward()
    ref = dict(dw=w.grad.numpy())
    if has_b:
        ref["db"] = b.grad.numpy()
    if cl:
        ref["dpos"] = dy.double().sum(0).numpy()
    return dict(x=x, dy=dy), ref, L


def _patch_launch(name, dtype, fill, det=True):
    lib = _lib()
    B, C, S, P, D, cl, has_b = PATCH[name]
    inp, _, L = _patch_case(name, dtype)
    x, dy = inp["x"].to("cuda", dtype), inp["dy"].to("cuda", dtype)
    ofill = fill if det else 0.0      # the default entry point accumulates into zeroed dw / db
    dw = _full(ofill, D, C, *P)
    db = _full(ofill, D) if has_b else None
    dpos = _full(fill, L, D) if cl else None
    Sa, Pa = lib.c_array(ctypes.c_int, S, 3, 1), lib.c_array(ctypes.c_int, P, 3, 1)
    head = (x.data_ptr(), lib.DTYPE[dtype], dy.data_ptr(), lib.DTYPE[dtype], dw.data_ptr(), lib.ptr(db), lib.ptr(dpos))
    if det:
        K = C * int(np.prod(P))
        ntiles = -(-L // min(256, 16384 // K))
        rows = B * max(1, min(ntiles, 1024 // B))
        nbytes = lib.load().lci_patch_embed_bwd_det_ws_bytes(B, C, D, len(S), Sa, Pa)
        assert nbytes == rows * D * (K + 1) * 4, (nbytes, rows)
        ws = _full(fill, nbytes // 4)
        lib.call("lci_patch_embed_bwd_det", *head, ws.data_ptr(), B, C, D, len(S), Sa, Pa, int(cl), lib.stream_of(x))
    else:
        lib.call("lci_patch_embed_bwd", *head, B, C, D, len(S), Sa, Pa, int(cl), lib.stream_of(x))
    torch.cuda.synchronize()
    out = dict(dw=dw)
    if has_b:
        out["db"] = db
    if cl:
        out["dpos"] = dpos
    return out


def _patch_bounds(name):
    _, _, _, _, _, cl, has_b = PATCH[name]
    b = dict(dw=1e-4)
    if has_b:
        b["db"] = 1e-4
    if cl:
        b["dpos"] = 1e-5
    return b


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", list(PATCH))
def test_patch_embed_bwd_det(name, dtype):
    runs = [_patch_launch(name, dtype, fill) for fill in FILLS]
    _check(f"{name}_{_ids(dtype)}", runs, _patch_case(name, dtype)[1], _patch_bounds(name))


def test_patch_embed_autograd_op_det():
    """kernels.patch_embed routes to the deterministic entry point under the mode: three runs, equal bits."""
    from long_context_biomedical_imaging_amd import kernels
    inp, ref, L = _patch_case("C1_vit_2d", F32)
    B, C, S, P, D, _, _ = PATCH["C1_vit_2d"]
    runs = []
    for fill in FILLS:
        _pollute(fill)
        w = torch.zeros(D, C, *P, device="cuda", requires_grad=True)
        b = torch.zeros(D, device="cuda", requires_grad=True)
        pos = torch.zeros(1, L, D, device="cuda", requires_grad=True)
        with kernels.deterministic_mode():
            y = kernels.patch_embed(inp["x"].cuda(), w, b, pos, channels_last_tokens=True)
        y.backward(inp["dy"].cuda())
        torch.cuda.synchronize()
        runs.append(dict(dw=w.grad, db=b.grad, dpos=pos.grad[0]))
    _check("C1_op", runs, ref, _patch_bounds("C1_vit_2d"))


# ------------------------------------------------------------------------------------------------ D: default mode
def test_default_mode_still_meets_the_bounds():
    """The default entry points on A1, B1 and C1 (f32 and bf16 where the case has both): the same fp64 bounds."""
    for dtype in DTYPES:
        _check(f"D_A1_{_ids(dtype)}", [_scan_launch("A1", dtype, FILLS[0], det=False)], _scan_ref("A1", dtype),
               _scan_bounds(dtype))
        _check(f"D_C1_{_ids(dtype)}", [_patch_launch("C1_vit_2d", dtype, FILLS[0], det=False)],
               _patch_case("C1_vit_2d", dtype)[1], _patch_bounds("C1_vit_2d"))
    name = "B1_bwd3_k3_bias"
    _check("D_B1", [_hyena_launch(name, FILLS[0], det=False)], _hyena_case(name)[1], _hyena_bounds(name))


# ------------------------------------------------------------------------------------------------ E: mixer modules
def _module_grads(build, x, cot):
    from long_context_biomedical_imaging_amd import kernels
    torch.manual_seed(1234)
    m = build().cuda()
    x = x.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16), kernels.deterministic_mode():
        out = m(x)
    out.float().backward(cot.cuda())
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    grads["input"] = x.grad
    return grads


@pytest.mark.parametrize("which", ["mamba", "hyena"])
def test_mixer_module_grads_bitwise(which):
    from long_context_biomedical_imaging_amd import hyena, mamba
    if which == "mamba":
        g = Golden("mamba_mixer")
        build = lambda: mamba.MambaVisionMixer(d_model=128, d_state=8, d_conv=3, expand=1)  # noqa: E731
    else:
        g = Golden("hyena_op")
        build = lambda: hyena.HyenaOperator(d_model=128, l_max=66000, filter_order=64, num_heads=2,  # noqa: E731
                                            num_blocks=1, short_filter_order=5, bidrectional=True, dropout=0.0,
                                            filter_dropout=0.0, activation="id")
    x, cot = g.t("in/x"), cotangents([g.t("out/0")])[0]
    a, b = _module_grads(build, x, cot), _module_grads(build, x, cot)
    assert a.keys() == b.keys() and len(a) > 3
    bad = [n for n in a if not torch.isfinite(a[n].float()).all() or not torch.equal(_bits(a[n]), _bits(b[n]))]
    assert not bad, f"{which}: gradients differ between two runs from one seed: {bad}"


# ------------------------------------------------------------------------------------------------ H: training steps
_SWIN = ["--encoder_name", "Swin", "--decoder_name", "UperNet3D", "--task_type", "seg", "--height", "32", "--width",
         "32", "--time", "32", "--no_in_channel", "1", "--no_out_channel", "2", "--Swin.size", "tiny",
         "--Swin.patch_size", "2", "2", "2"]
TRAIN = {
    "swin_mamba_w4": _SWIN + ["--Swin.window_size", "4", "4", "4", "--Swin.use_mamba", "True"],
    "swin_hyena_w8": _SWIN + ["--Swin.window_size", "8", "8", "8", "--Swin.use_hyena", "True"],
    "vit_mamba": ["--encoder_name", "ViT", "--decoder_name", "ViTUNETR", "--task_type", "seg", "--height", "16",
                  "--width", "16", "--time", "16", "--no_in_channel", "1", "--no_out_channel", "2", "--ViT.size",
                  "small", "--ViT.patch_size", "2", "2", "2", "--ViT.use_mamba", "True"],
}
# Parameters upstream of a torch op found nondeterministic (none: every parameter is compared)
TRAIN_EXCLUDED = {"swin_mamba_w4": (), "swin_hyena_w8": (), "vit_mamba": ()}


def _train_twice_two_steps(name):
    from long_context_biomedical_imaging_amd import config, model_base, trainer
    cfg = config.parse_config(TRAIN[name] + ["--optim_type", "adam", "--optim.lr", "1e-3", "--batch_size", "2",
                                             "--deterministic", "--use_amp"])
    assert cfg.deterministic
    dev = torch.device("cuda", 0)
    x, y = trainer.synthetic_batch(cfg, 2, dev, 4321)
    res = []
    for _ in range(2):
        torch.manual_seed(77)
        model = model_base.EncoderDecoderModel(cfg, cfg.encoder_name, cfg.decoder_name, cfg.no_in_channel,
                                               cfg.no_out_channel).to(dev).train()
        ts = trainer.TrainStep(model, cfg, dev, ddp=False)
        for _ in range(2):
            loss = ts.step(x, y)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        res.append({n: p.detach().clone() for n, p in model.named_parameters()})
    return res


@pytest.mark.parametrize("name", list(TRAIN))
def test_two_training_steps_bitwise(name):
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        a, b = _train_twice_two_steps(name)
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    bad = [n for n in a if n not in TRAIN_EXCLUDED[name]
           and (not torch.isfinite(a[n]).all() or not torch.equal(_bits(a[n]), _bits(b[n])))]
    assert not bad, f"{name}: {len(bad)} of {len(a)} parameters differ after two deterministic steps: {bad[:12]}"
