"""The wide attention forward (csrc/attention.hip, attn_fwd_hs4_kernel: 128 queries per wave) without a GPU: the
host-side choice between it and attn_fwd_hs_kernel (lci_attn_fwd_pick), and the same ISA guards
tests/test_attention_isa_cpu.py applies to the other placed-stream kernels (no allocator copies or spills in its
loops, no scratch, no MFMA hazard the compiler could not see)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "long_context_biomedical_imaging_amd", "csrc", "attention.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME = "attn_fwd_hs4_kernel"
WIDE_Q = 512   # queries per workgroup of the wide kernel (4 waves x 128)


def _pick():
    from long_context_biomedical_imaging_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liblci.so not built (python -m long_context_biomedical_imaging_amd.build_lib)")
    return _lib.load().lci_attn_fwd_pick


def test_pick_pinned_points():
    pick = _pick()
    assert pick(2, 65536, 6, 256) == 1      # 1536 workgroups: 6 full rounds of 256 CUs
    assert pick(2, 32768, 6, 256) == 1      # 768: 3 full rounds
    assert pick(2, 16384, 6, 256) == 0      # 384 would be 1.5 rounds
    for L in (1, 33, 81, 511):              # L < 512: one workgroup per (b, h)
        assert pick(2, L, 6, 256) == 0
    assert pick(1, 512, 1, 256) == 0


def test_pick_never_wide_below_one_round_or_with_a_long_tail():
    pick = _pick()
    for n_cu in (64, 240, 256, 304):
        for B in (1, 2, 3, 8):
            for H in (1, 3, 6, 12):
                for L in (1, 500, 512, 513, 4096, 10000, 16384, 20000, 32768, 65536, 100000):
                    W = B * H * ((L + WIDE_Q - 1) // WIDE_Q)
                    got = pick(B, L, H, n_cu)
                    assert got in (0, 1)
                    rounds = (W + n_cu - 1) // n_cu
                    want = int(W >= n_cu and 10 * W >= 9 * rounds * n_cu)
                    assert got == want, (B, L, H, n_cu, W)
                    if W < n_cu:
                        assert got == 0
    assert pick(2, 65536, 6, 0) == 0        # unknown device: narrow


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    from long_context_biomedical_imaging_amd import build_lib
    out = tmp_path_factory.mktemp("isa_wide") / "attention.s"
    cmd = [HIPCC, *build_lib.FLAGS, *build_lib.DEVICE_FLAGS, *build_lib.FILE_FLAGS.get("attention.hip", []),
           "--cuda-device-only", "-S", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = out.read_text()
    m = re.search(r"^(_Z\S*" + NAME + r"\S*):", isa, re.M)
    assert m, f"{NAME} not in the ISA"
    return isa[m.end():isa.index(".Lfunc_end", m.end())]   # (blocks may be laid out after an s_endpgm)


def _loops(body):
    """Every loop's instruction text: its header block and the blocks annotated as inside it."""
    blocks = re.split(r"^(?=\.LBB\d+_\d+:)", body, flags=re.M)
    out = []
    for blk in blocks:
        m = re.match(r"\.L(BB\d+_\d+):.*Loop Header", blk)
        if not m:
            continue
        hid = m.group(1)
        out.append("\n".join(b for b in blocks
                             if b is blk or re.match(r"\.LBB\d+_\d+:.*in Loop: Header=" + hid + r"\b", b)))
    return out


def test_no_allocator_copies_in_loops_and_no_scratch(body):
    loops = _loops(body)
    assert loops, f"{NAME}: no loop found"
    for lp in loops:
        code = "\n".join(l for l in lp.splitlines() if not l.strip().startswith(";"))
        bad = re.findall(r"^\s*(v_accvgpr_(?:read|write|mov)_b32|scratch_\w+|buffer_store_dword\w*)\b.*$", code, re.M)
        assert not bad, f"{NAME}: allocator copies / spills inside a loop: {bad[:5]}"
    assert "scratch_" not in body, f"{NAME}: scratch spills"


def test_stream_shape(body):
    """The 4-tile unrolled loop: per 64-key tile 64 large MFMAs (32 per half) and 16 row-sum MFMAs against the narrow
    kernel's 24 fragment reads, 4 staging stores and one barrier."""
    main = max(_loops(body), key=len)
    code = "\n".join(l for l in main.splitlines() if not l.strip().startswith(";"))
    n = lambda pat: len(re.findall(pat, code))   # noqa: E731
    assert n(r"v_mfma_f32_32x32x16_bf16") == 4 * 64
    assert n(r"v_mfma_f32_16x16x32_bf16") == 4 * 16
    assert n(r"\bds_read_b128\b") == 4 * 8 and n(r"\bds_read_b64_tr_b16\b") == 4 * 16
    assert n(r"\bds_write_b128\b") == 4 * 4
    assert n(r"\bs_barrier\b") == 4
    assert n(r"\bv_exp_f32\b") == 4 * 2 * 64 and n(r"\bv_cvt_pk_bf16_f32\b") == 4 * 2 * 32


def test_no_mfma_hazards(body):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hazards
    ins = isa_hazards.parse(body.splitlines())
    hits = isa_hazards.scan(ins)
    assert not hits, f"{NAME}: " + "; ".join(f"{k} ws={ws}: `{ins[i][0]}` -> `{ins[j][0]}`" for k, i, j, ws in hits[:5])
