"""The wide attention-backward dQ kernel (csrc/attention.hip, attn_bwd_dq_hs4_kernel: 128 queries per wave) without a
GPU: the host-side choice between it and attn_bwd_dq_hs_kernel (lci_attn_bwd_dq_pick, the rule of lci_attn_fwd_pick),
its VALU placement table against the generator (tools/gen_dq_sched.py --nqb 4) and the generator's own rules, and the
ISA guards tests/test_attention_isa_cpu.py applies to the narrow kernels (through that module's helpers): no scratch,
no allocator copies in the tile loop, no MFMA hazard the compiler could not see. The fallback entry
(attn_bwd_dq_hsfb_kernel, the narrow body behind an early exit) gets the same guards."""
import os
import re
import subprocess
import sys

import pytest

import test_attention_isa_cpu as isa_cpu

ROOT = isa_cpu.ROOT
SRC = isa_cpu.SRC
GEN = os.path.join(ROOT, "tools", "gen_dq_sched.py")
WIDE = "attn_bwd_dq_hs4_kernel"
FALLBACK = "attn_bwd_dq_hsfb_kernel"
WIDE_Q = 512   # queries per workgroup of the wide kernel (4 waves x 128)

isa = isa_cpu.isa   # the module-scoped fixture: one gfx950 compile of attention.hip


def _lib():
    from long_context_biomedical_imaging_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liblci.so not built (python -m long_context_biomedical_imaging_amd.build_lib)")
    return _lib.load()


def test_pick_pinned_points():
    pick = _lib().lci_attn_bwd_dq_pick
    assert pick(2, 65536, 6, 256) == 1      # 1536 workgroups: 6 full rounds of 256 CUs
    assert pick(2, 32768, 6, 256) == 1      # 768: 3 full rounds
    assert pick(2, 16384, 6, 256) == 0      # 384 would be 1.5 rounds
    assert pick(4, 512, 64, 256) == 1       # 256 workgroups of one tile row each
    assert pick(1, 512, 1, 256) == 0
    assert pick(2, 65536, 6, 0) == 0        # unknown device: narrow


def test_pick_is_the_forward_rule():
    lib = _lib()
    for n_cu in (64, 240, 256, 304):
        for B in (1, 2, 3, 8):
            for H in (1, 3, 6, 12):
                for L in (1, 500, 512, 513, 4096, 10000, 16384, 20000, 32768, 65536, 100000):
                    W = B * H * ((L + WIDE_Q - 1) // WIDE_Q)
                    rounds = (W + n_cu - 1) // n_cu
                    want = int(W >= n_cu and 10 * W >= 9 * rounds * n_cu)
                    assert lib.lci_attn_bwd_dq_pick(B, L, H, n_cu) == want, (B, L, H, n_cu, W)
                    assert lib.lci_attn_fwd_pick(B, L, H, n_cu) == want


def test_workspace_holds_the_flags():
    """(B, H, 2, L) f32 row constants, then one int32 per wide workgroup, rounded up to 256 bytes."""
    ws = _lib().lci_attn_bwd_ws_bytes
    for B, H, L in ((1, 1, 512), (1, 1, 77), (1, 2, 300), (2, 3, 1100), (2, 6, 65536)):
        need = 4 * (B * H * 2 * L + B * H * ((L + WIDE_Q - 1) // WIDE_Q))
        assert ws(B, H, L) == (need + 255) // 256 * 256


def _gen(*args):
    r = subprocess.run([sys.executable, GEN, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_generator_default_is_the_committed_narrow_table():
    out = _gen()
    assert out.startswith("constexpr unsigned char DQ_SCHED[24][4] = {")
    assert out.strip() in open(SRC).read(), "DQ_SCHED in attention.hip is not the generator's output, byte for byte"


def _table(text, name, ng):
    m = re.search(r"constexpr unsigned char " + name + r"\[" + str(ng) + r"\]\[4\] = \{(.*?)\};", text, re.S)
    assert m, f"{name} not found"
    vals = [int(v, 16) for v in re.findall(r"0x([0-9a-f]{2})", m.group(1))]
    assert len(vals) == 4 * ng
    return [vals[4 * g:4 * g + 4] for g in range(ng)]


def test_wide_table_is_the_generator_output_and_keeps_its_rules():
    out = _gen("--nqb", "4")
    src = open(SRC).read()
    assert out.strip() in src, "DQ4_SCHED in attention.hip is not the output of gen_dq_sched.py --nqb 4"
    NG, NQB = 48, 4
    tab = _table(src, "DQ4_SCHED", NG)
    # the periodic stream as (gap, position, kind, block, index); a block's ops before its first gap belong to the
    # previous half (the last block wraps), so their time is one period later
    when = {}
    stream = []
    for g, row_ in enumerate(tab):
        seen_pad = False
        for o, c in enumerate(row_):
            if c == 0xFF:
                seen_pad = True
                continue
            assert not seen_pad, f"gap {g}: an op after a pad entry"
            kind, qb, i = "EMC"[c >> 6], (c >> 4) & 3, c & 15
            t = g if g >= 12 * qb + 5 else g + NG
            assert (kind, qb, i) not in when, f"{kind}{qb}.{i} placed twice"
            when[(kind, qb, i)] = (t, o)
            stream.append((g, o, kind, qb, i))
    for qb in range(NQB):
        for i in range(16):
            assert ("E", qb, i) in when and ("M", qb, i) in when
        for j in range(8):
            assert ("C", qb, j) in when
    for g, row_ in enumerate(tab):
        assert sum(1 for c in row_ if c != 0xFF and c >> 6 == 0) <= 2, f"gap {g}: more than 2 exp2"
    for qb in range(NQB):
        s_end, p_end, dq0 = 12 * qb + 3, 12 * qb + 7, 12 * qb + 20
        for i in range(16):
            tE, tM = when[("E", qb, i)], when[("M", qb, i)]
            assert tE[0] >= s_end + 2, f"E{qb}.{i} too soon after the S chain"
            assert tM[0] >= p_end + 2 and tM[0] > tE[0], f"M{qb}.{i}"
        for j in range(8):
            tC = when[("C", qb, j)]
            assert tC > when[("M", qb, 2 * j)] and tC > when[("M", qb, 2 * j + 1)], f"C{qb}.{j} before its multiplies"
            # packs before the MFMAs that read them: k-step 0 (C 0-3) at dq0, dq0 + 1; k-step 1 (C 4-7) at dq0 + 2, + 3
            assert tC[0] < (dq0 if j < 4 else dq0 + 2), f"C{qb}.{j} after the dQ^T MFMA that reads its pack"
            # ... and not while the previous user of the pack registers (block qb - 2, same set) still reads them
            assert tC[0] > dq0 - 24 + 3
        last = max(when[(k, qb, i)][0] for k in "EM" for i in range(16))
        last = max(last, max(when[("C", qb, j)][0] for j in range(8)))
        assert last < 12 * qb + 24, f"block {qb} still runs when block {qb + 2}'s chains rewrite its register set"
    # no exp directly before an op that reads its result (the periodic stream: gap 47 before gap 0)
    for a, b in zip(stream, stream[1:] + stream[:1]):
        if a[2] == "E" and b[2] == "M" and a[3:] == b[3:]:
            raise AssertionError(f"gap {b[0]}: M{b[3]}.{b[4]} directly after its exp")


@pytest.mark.parametrize("name", (WIDE, FALLBACK))
def test_no_allocator_copies_in_placed_loops(isa, name):
    isa_cpu.test_no_allocator_copies_in_placed_loops(isa, name)


@pytest.mark.parametrize("name", (WIDE, FALLBACK))
def test_no_mfma_hazards(isa, name):
    isa_cpu.test_no_mfma_hazards(isa, name)


def _meta(isa, name, key):
    m = re.search(r"\.amdhsa_kernel \S*" + name + r"\S*\s.*?\.end_amdhsa_kernel", isa, re.S)
    assert m, f"{name}: no kernel descriptor"
    v = re.search(r"\." + key + r"\s+(\d+)", m.group(0))
    assert v, f"{name}: {key} not in the kernel descriptor"
    return int(v.group(1))


def test_wide_registers_and_scratch(isa):
    """No scratch; arch + acc registers within the 512 of one wave per SIMD (the descriptor's next_free_vgpr counts
    the unified file: the arch registers, rounded up to the allocation granule, plus the AGPRs)."""
    assert _meta(isa, WIDE, "amdhsa_private_segment_fixed_size") == 0
    assert _meta(isa, WIDE, "amdhsa_next_free_vgpr") <= 512
    assert _meta(isa, WIDE, "amdhsa_accum_offset") <= 256
    assert "scratch_" not in isa_cpu._kernel_body(isa, WIDE)


def test_wide_stream_shape(isa):
    """The 4-tile unrolled loop: per 64-key tile 96 MFMAs per half pair (48 + 48) against the narrow kernel's 32
    fragment reads (8 row + 8 transposed per half), 4 staging stores, 4 staging loads and one barrier."""
    main = max(isa_cpu._loops(isa_cpu._kernel_body(isa, WIDE)), key=len)
    code = "\n".join(l for l in main.splitlines() if not l.strip().startswith(";"))
    n = lambda pat: len(re.findall(pat, code))   # noqa: E731
    assert n(r"v_mfma_f32_32x32x16_bf16") == 4 * 96
    assert n(r"\bds_read_b128\b") == 4 * 16 and n(r"\bds_read_b64_tr_b16\b") == 4 * 16
    assert n(r"\bds_write_b128\b") == 4 * 4 and n(r"\bbuffer_load_dwordx4\b") == 4 * 4
    assert n(r"\bs_barrier\b") == 4
    assert n(r"\bv_exp_f32\b") == 4 * 2 * 64 and n(r"\bv_mul_f32\b") == 4 * 2 * 64
    assert n(r"\bv_cvt_pk_bf16_f32\b") == 4 * 2 * 32
