// ViT full self-attention (SABlock, backbone_vit.py:191-203) as flash attention for gfx950.
//
// Replaces:  att = softmax(einsum("blxd,blyd->blxy", q, k) * scale); x = einsum("bhxy,bhyd->bhxd", att, v)
// Layout:    q/k/v are read in place from the packed qkv Linear output (B, L, 3*H*64) bf16, channel
//            order (qkv, head, d) (backbone_vit.py:168); O is written as (B, L, H*64) = out_rearrange.
//            The L x L score matrix is never materialised; the forward keeps lse2 = log2(sum exp) per row.
//
// Three kernels, each one wave per SIMD (4-wave workgroups, the whole register file per wave) running a hand-placed
// stream of v_mfma_f32_32x32x16_bf16 and softmax VALU (inline asm, fixed order):
// Forward:   attn_key_norm_kernel (per-64-key-tile max ||k||) + attn_fwd_hs_kernel: 64 queries per wave on the MFMA
//            lane, S^T = K.Q~^T, lane-local max-free softmax on tiles the key-norm bound proves safe (exact online
//            softmax otherwise), O^T += V^T.P^T with P straight from the S accumulators. Where the grid still fills
//            the chip (lci_attn_fwd_pick: the metric shape, L = 65536) attn_fwd_hs4_kernel runs instead: the same
//            stream with 128 queries per wave, half the K | V staging, LDS reads and barriers per MFMA, bitwise the
//            same O and lse2.
// Backward:  (1) attn_bwd_delta_kernel: delta = rowsum(dO*O), written with -lse2 as the chains' row constants;
//            (2) attn_bwd_dkdv_hs_kernel: 64 keys per wave on the lane, sweeps query tiles: S, dP recomputed,
//            dV^T += dO^T.P, dK^T += Q^T.dS; where both grids still fill the chip (lci_attn_bwd_dkdv_pick: the metric
//            shape) the first 384 W keys go to attn_bwd_dkdv_hs3_kernel instead: the same stream with 96 keys per
//            wave, two thirds of the LDS reads per MFMA, bitwise the same dK and dV; (3) attn_bwd_dq_hs_kernel: 64 queries per wave, sweeps key tiles:
//            S^T, dP^T, dQ^T += K^T.dS^T; where the grid still fills the chip (lci_attn_bwd_dq_pick, the forward's rule)
//            attn_bwd_dq_hs4_kernel instead: 128 queries per wave on one shared softmax shift per lane, half the
//            K | V staging, LDS reads and barriers per MFMA (workgroups whose lse2 spread forbids the shared shift
//            are left to attn_bwd_dq_hsfb_kernel, the narrow stream). No atomics: results are bitwise reproducible.
// Superseded variants (2 waves per SIMD, 16x16x32 shapes, d-major Q/dO staging, MFMA row sums, timing probes) were
// removed in round 5; their same-box A/B records are kept in profiles/r0[1-4]_attn_*.
#include "common.hpp"

#include <type_traits>
#include <utility>

namespace lci {

constexpr int DH = 64;        // head dim (ViT-small/base: 384/6, 768/12)
constexpr int KT = 64;        // keys (or queries) per LDS tile
constexpr float NEG_BIG = -1.0e30f;

struct AttnArgs {
  const bf16* q; const bf16* k; const bf16* v;    // base pointers of head 0, batch 0
  const bf16* o; const bf16* dout;                 // bwd only
  bf16* out;                                       // fwd: O ; bwd dq kernel: dQ
  bf16* dk; bf16* dv;                              // bwd dkdv kernel
  float* lse2;                                     // (B, H, L)
  float* delta;                                    // bwd: (B, H, 2, L) negated row constants [-lse2 | -delta]
  long long bs_q, bs_k, bs_v, bs_o, bs_do, bs_out, bs_dk, bs_dv;   // batch strides (elements)
  int rs_q, rs_k, rs_v, rs_o, rs_do, rs_out, rs_dk, rs_dv;         // token (row) strides (elements)
  int hs;                                          // head stride (elements) in every tensor (= 64)
  int H, L;
  float c;                                         // scale * log2(e)
  float scale;
  int k0;                                          // bwd dkdv kernel: first key of its grid (keys below: the wide kernel's)
};

// Per-64-key-tile bound on |k|: knorm[b][h][t] = max_{key in tile t} ||k_key||_2 (f32 of the bf16 keys).
// One wave per tile, lane = key. Used by the forward's max-free fast path (below).
__global__ __launch_bounds__(256) void attn_key_norm_kernel(AttnArgs a, float* knorm, int nkt) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int hh = blockIdx.y, b = blockIdx.z;
  if (t >= nkt) return;
  const int key = t * KT + lane;
  float ss = 0.f;
  if (key < a.L) {
    const bf16* kp = a.k + b * a.bs_k + (long long)key * a.rs_k + hh * a.hs;
#pragma unroll
    for (int c = 0; c < DH / 8; ++c) {
      const bf16x8 v = *(const bf16x8*)(kp + 8 * c);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += to_f32(v[j]) * to_f32(v[j]);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ss = fmaxf(ss, __shfl_xor(ss, off));
  if (lane == 0) knorm[((long long)b * a.H + hh) * nkt + t] = sqrtf(ss);
}

// Max-free softmax (forward): p = exp2(s~ - m) against a reference m that is only moved when it must be. A tile is
// "safe" when every row's bound ||q~|| * max||k|| - m <= 64 (q~ = c q, bf16; knorm per tile from
// attn_key_norm_kernel): then p <= 2^64, which f32 sums and bf16 P carry exactly as well as p <= 1, and the tile
// needs no row max at all. Unsafe tiles (and the first) take the exact path: row max, lazy re-base of m
// (alpha = exp2(-d) on O and l). The result is the same softmax; only the reference point of the exponent differs.
constexpr float SAFE_EXP2 = 64.f;
// --------------------------------------------------------------------------- backward: delta
// delta[b,h,q] = sum_d dO[b,q,h,d] * O[b,q,h,d]; 8 threads per (q, h) row, 16 B each. Written negated, next to the
// negated lse2, as the backward kernels' row constants: ws[b][h][0][q] = -lse2, ws[b][h][1][q] = -delta (the chains'
// initial accumulators; the dK/dV kernel stages a tile's 64 + 64 of them with two contiguous loads).
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(AttnArgs a) {
  const int tid = threadIdx.x;
  const int row = blockIdx.x * 32 + (tid >> 3), ch = tid & 7;
  const int hh = blockIdx.y, b = blockIdx.z;
  float acc = 0.f;
  if (row < a.L) {
    const bf16x8 o = *(const bf16x8*)(a.o + b * a.bs_o + (long long)row * a.rs_o + hh * a.hs + ch * 8);
    const bf16x8 d = *(const bf16x8*)(a.dout + b * a.bs_do + (long long)row * a.rs_do + hh * a.hs + ch * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += to_f32(o[j]) * to_f32(d[j]);
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  acc += __shfl_xor(acc, 4);
  if (ch == 0 && row < a.L) {
    float* ws = a.delta + ((long long)b * a.H + hh) * 2 * a.L;
    ws[row] = -a.lse2[((long long)b * a.H + hh) * a.L + row];
    ws[a.L + row] = -acc;
  }
}

// ------------------------------------- backward: dK, dV kernel, one wave per SIMD, placed MFMA / VALU / LDS stream
// VERDICT r03 item 1. A workgroup = 4 waves (one per SIMD, the whole register file each), a wave owns 64 keys (two
// key blocks of 32, key on the MFMA lane), so every Q / dO fragment read from LDS feeds two key blocks: half the LDS
// bytes per MFMA of the 32-key kernels. Per 32-query half-tile and wave: 32 v_mfma_f32_32x32x16_bf16 (S and dP
// chains 8 + 8, dV^T 8, dK^T 8) against 32 exp2 + 32 multiplies + 32 conversions (P = exp2(S~ - lse2) and dS =
// P (dP - delta) need no subtract: -lse2 / -delta are the chains' initial accumulators, read as f32x4 from the tile's
// row-constant rows) and 40 LDS reads: one MFMA gap holds 1 exp2, 1 multiply, 0-2 conversions and 0-2 LDS reads
// (MI355X_MICROARCH.md "one wave per SIMD": <= 5 fillers, <= 1 transcendental per 32x32x16 gap).
// Software pipeline: key block 1 runs half a period behind key block 0, so each block's S / dP registers are
// produced, consumed and refilled in turn and every gap pairs one block's MFMAs with the other block's VALU.
// Per half-tile p, four segments of 8 MFMA gaps:
//   seg A: S chain, dP chain kb0 (half p)     || VALU kb1 (half p-1), elements 8-15
//   seg B: dV^T / dK^T kb1 (half p-1)        || VALU kb0 (half p), elements 0-7  | LDS: dO^T / Q^T of half p
//   seg C: S chain, dP chain kb1 (half p)     || VALU kb0 (half p), elements 8-15 | LDS: dO^T / Q^T, Q rows of p+1
//   seg D: dV^T / dK^T kb0 (half p)          || VALU kb1 (half p), elements 0-7  | LDS: row constants, dO rows of p+1
// Every MFMA and every exp2 / multiply / conversion of the loop is its own `asm volatile` statement, so the stream
// is issued exactly in the order written (the compiler only allocates registers and inserts the LDS waits); the
// dV / dK accumulators (128) and the K / V fragments (64) are "a" operands (the AGPR half of the file), the VALU
// working set (~220) stays in the arch VGPRs. Hazards the compiler cannot see into asm are covered by the placement
// (gfx950 wait states, measured from the compiler's own insertions: MFMA -> VALU read 12, VALU -> MFMA A/B read 2,
// exp -> dependent VALU 1, MFMA C read -> overwrite 7): a chain's last S MFMA is 4 gaps before the first exp of it,
// its last dP MFMA 3 gaps before the first multiply, a pack 2+ gaps before its MFMA, a fragment reloaded 2 gaps after
// its last MFMA read.
// Q / dO tiles of 64 queries arrive in a 3-slot LDS ring (128-B rows, 16-B chunk XOR ((r >> 2) & 3 | ((r >> 1) & 1)
// << 2): conflict-free for the 32x32 row reads and the transposed reads), staged through registers one tile ahead;
// one barrier per tile, between its two halves (half 1's seg C / D read the next tile).
constexpr int HS_NW = 4;
__device__ __forceinline__ int sw128(int row, int col) {
  const int g = ((row >> 2) & 3) | (((row >> 1) & 1) << 2);
  return row * DH + ((((col >> 3) ^ g) << 3) | (col & 7));
}
// LDS-DMA from a buffer resource: every lane's 16 (4) bytes at voff + soff land at LDS byte address lds + 16 (4) * lane;
// rows past the resource's range read as zero. Issued from asm so that the compiler neither tracks it as an LDS write
// nor counts it in its vmcnt waits (completion is waited for explicitly before the barrier that publishes the tile).
__device__ __forceinline__ void hs_dma16(rsrc_t r, int voff, int soff, unsigned lds) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(r), "s"(lds), "s"(soff) : "memory");
}
__device__ __forceinline__ void hs_dma4(rsrc_t r, int voff, int soff, unsigned lds) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(r), "s"(lds), "s"(soff) : "memory");
}
// 16-byte (4-byte) buffer load into AGPRs, issued from asm: the compiler does not count it in its vmcnt waits (it would
// wait for every load in flight before the first use of any), so the use must be preceded by an explicit hs_vmcnt
__device__ __forceinline__ u32x4 hs_ld16(rsrc_t r, int voff, int soff) {
  u32x4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=a"(v) : "v"(voff), "s"(r), "s"(soff) : "memory");
  return v;
}
__device__ __forceinline__ uint32_t hs_ld4(rsrc_t r, int voff, int soff) {
  uint32_t v;
  asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=a"(v) : "v"(voff), "s"(r), "s"(soff) : "memory");
  return v;
}
template <int N>
__device__ __forceinline__ void hs_vmcnt() {   // s_waitcnt vmcnt(N), lgkmcnt / expcnt untouched
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}
// Give a value an AGPR home (one copy, here): every later use is an asm "a" operand, so the allocator needs no copy
// next to a (hazard-blind) asm MFMA that reads it
#define HS_TO_AGPR(x) asm volatile("" : "=a"(x) : "0"(x))
// the compiler loses track of x's value (an asm output): zero-initialised fragments and accumulators must not become
// constants it rematerialises with a VALU move right next to the asm MFMA that reads them (it cannot see the hazard)
#define HS_OPAQUE(x) asm volatile("" : "+v"(x))
// keep x's registers allocated up to here: a chain's row-constant initial accumulator is read by the MFMA pipeline
// after issue, so nothing may reuse those registers within the next seven wait states
#define HS_KEEP(x) asm volatile("" ::"v"(x))
#define HS_EXP(x) asm volatile("v_exp_f32 %0, %0" : "+v"(x))
#define HS_MUL(p, e) asm volatile("v_mul_f32 %0, %1, %0" : "+v"(p) : "v"(e))
#define HS_CVT(w, x0, x1) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(x0), "v"(x1))
// accumulate into AGPRs (dV^T / dK^T), A and B from VGPRs
#define HS_MFMA_G(acc, A, B) \
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(A), "v"(B))
// S / dP chains: B = the K / V fragment in AGPRs; the first step reads the row constants as C (separate registers)
#define HS_MFMA_C0(d, A, B, C) \
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(A), "a"(B), "v"(C))
#define HS_MFMA_C(d, A, B) \
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(d) : "v"(A), "a"(B))
// the same with B in arch VGPRs (attn_bwd_dkdv_hs3_kernel: its third key block's fragments, the AGPR half being full)
#define HS_MFMA_C0V(d, A, B, C) \
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(A), "v"(B), "v"(C))
#define HS_MFMA_CV(d, A, B) \
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(d) : "v"(A), "v"(B))

// s_waitcnt lgkmcnt(0) with vmcnt / expcnt left at their maxima (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] |
// lgkmcnt[11:8] | vmcnt[15:14])
constexpr unsigned LGKM0_WAIT = 0xC07F;
// 16- / 4-byte LDS stores of AGPR data at a lane address + immediate (asm: no VGPR copy; completion is implied by the
// compiler's in-order lgkmcnt waits for later reads)
template <int OFF>
__device__ __forceinline__ void hs_st16(unsigned addr, const u32x4& v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "a"(v), "i"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void hs_st4(unsigned addr, uint32_t v) {
  asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(addr), "a"(v), "i"(OFF) : "memory");
}
// the same from / to arch VGPRs, for a kernel whose AGPR half is full (attn_bwd_dq_hs4_kernel)
__device__ __forceinline__ u32x4 hs_ld16v(rsrc_t r, int voff, int soff) {
  u32x4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v) : "v"(voff), "s"(r), "s"(soff) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ void hs_st16v(unsigned addr, const u32x4& v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "i"(OFF) : "memory");
}
// f(integral_constant<int, g>) for every gap g of a half, unrolled by pack expansion (a `#pragma unroll` loop of 40+
// gaps of a placed stream is past the loop unroller's limit and silently stays a loop)
template <class F, int... G>
__device__ __forceinline__ void hs_for_gaps(F&& f, std::integer_sequence<int, G...>) {
  (f(std::integral_constant<int, G>{}), ...);
}

// ---- what the six placed kernels share. These helpers only compute values: where a kernel waits (hs_vmcnt) and
// where it moves fragments to AGPRs (HS_TO_AGPR) is part of its measured build and stays written in the kernel. The
// register allocation of a placed loop follows the order of the prologue's statements, down to independent ones, and
// the form the compiler sees them in before inlining: a helper keeps the statements it replaced, in their order
// (the thread decomposition, the fragment offsets and the forward's prologue and exact path moved registers or
// streams when shared, and stay in the kernels; DESIGN.md "Attention: shared pieces").
// The tile ring: 4 slots of two 64-row tiles (Q | dO or K | V, 128-B sw128 rows), tile t in slot t & 3. It fills
// exactly 64 KB, so every fragment read of every slot is one lane register + a 16-bit DS immediate.
constexpr int HS_TILE_B = KT * DH * 2;
constexpr int HS_SLOT_B = 2 * HS_TILE_B;
constexpr int HS_NSLOT = 4;
static_assert((HS_NSLOT & (HS_NSLOT - 1)) == 0, "ring slot of tile t is t & (HS_NSLOT - 1)");
static_assert(HS_NSLOT * HS_SLOT_B == 65536, "ring reachable by DS immediates");

// A wave's share of staging a ring of (X | Y) tiles of a head: rows 16 wave .. 16 wave + 15 of each tile as two 1-KB
// pieces of 8 rows (lane l -> row l >> 3 of the piece, physical 16-B chunk l & 7, fetched from the logical chunk
// (l & 7) ^ g(row) of the sw128 swizzle). Operations 0-3 of a tile: X piece 0, 1, Y piece 0, 1. Rows >= L read as zero.
struct HsRing {
  rsrc_t rx, ry;
  int x0, x1, y0, y1;   // the lane's byte offset within a tile, per operation
  int rs2x, rs2y;       // row strides in bytes
  unsigned lds0;        // LDS address of the ring
  int wave;
  // byte offset of tile t in its tensor: unsigned, tiles a few past the last are addressed (out of range: zeros) and
  // the entry points bound (L + 6 KT) rows by 2^31 bytes
  static __device__ __forceinline__ int toff(int t, int rs2) { return (int)((uint32_t)t * KT * (uint32_t)rs2); }
  __device__ __forceinline__ rsrc_t rsrc(int i) const { return i < 2 ? rx : ry; }
  __device__ __forceinline__ int voff(int i) const { return i == 0 ? x0 : i == 1 ? x1 : i == 2 ? y0 : y1; }
  __device__ __forceinline__ int soff(int t, int i) const { return toff(t, i < 2 ? rs2x : rs2y); }
  // operation i of tile t straight into the tile's ring slot by LDS-DMA (the prologue)
  __device__ __forceinline__ void dma(int t, int i) const {
    const unsigned sb = lds0 + (unsigned)((t & (HS_NSLOT - 1)) * HS_SLOT_B);
    hs_dma16(rsrc(i), voff(i), soff(t, i), sb + (i >> 1) * HS_TILE_B + 2048 * wave + (i & 1) * 1024);
  }
};
// buffer resource over rows 0 .. L-1 (DH bf16 each, row stride rs2 bytes) of a head's tensor
__device__ __forceinline__ rsrc_t hs_rows_rsrc(const bf16* p, int rs2, int L) {
  return make_rsrc(p, (uint32_t)(L - 1) * (uint32_t)rs2 + DH * 2);
}
// (the resources are the caller's, made in its own order: the dK/dV kernel makes its row-constant resource between)
__device__ __forceinline__ HsRing hs_ring(rsrc_t rx, int rs2x, rsrc_t ry, int rs2y, int lane, int wave,
                                          const char* smem) {
  HsRing r;
  r.rx = rx;
  r.ry = ry;
  r.rs2x = rs2x;
  r.rs2y = rs2y;
  // row = 16 wave + 8 j + prow (piece j = 0, 1): g(row) = ((row >> 2) & 3) | ((row >> 1) & 1) << 2 = (2j + (prow >> 2))
  // | ((prow >> 1) & 1) << 2
  const int prow = lane >> 3;
  const int pch0 = (lane & 7) ^ ((prow >> 2) | ((prow >> 1) & 1) << 2);
  const int pch1 = (lane & 7) ^ ((2 + (prow >> 2)) | ((prow >> 1) & 1) << 2);
  r.x0 = (16 * wave + prow) * r.rs2x + 16 * pch0, r.x1 = (16 * wave + 8 + prow) * r.rs2x + 16 * pch1;
  r.y0 = (16 * wave + prow) * r.rs2y + 16 * pch0, r.y1 = (16 * wave + 8 + prow) * r.rs2y + 16 * pch1;
  r.lds0 = (unsigned)(uintptr_t)(LCI_LDS char*)smem;
  r.wave = wave;
  return r;
}

// B-operand fragments of the backward kernels' operand pairs (K | V or Q | dO), one 32-row block: xf[ks] / yf[ks] =
// x / y[row][16 ks + 8 h .. + 7] of the head's tensors (row strides rs_x, rs_y), zeros for a row past L, x prescaled
// by c into the exp2 domain and rounded to bf16 again. The caller waits for the loads (hs_vmcnt) and moves the
// fragments to AGPRs where its own stream wants that.
__device__ __forceinline__ void hs_load_b2(bf16x8 (&xf)[4], bf16x8 (&yf)[4], const bf16* xp, int rs_x, const bf16* yp,
                                           int rs_y, int row, int L, int h, float c) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    if (row < L) {
      xf[ks] = *(const bf16x8*)(xp + (long long)row * rs_x + 16 * ks + 8 * h);
      yf[ks] = *(const bf16x8*)(yp + (long long)row * rs_y + 16 * ks + 8 * h);
    } else {
      xf[ks] = bf16x8{};
      yf[ks] = bf16x8{};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) xf[ks][j] = to_bf16(to_f32(xf[ks][j]) * c);
  }
}
// Row constants of the next half by DPP (LCI_DKDV_DPPRC=1): one ds_read_b32 per constant row set (lane l holds the
// constant of register l & 15 of its half-wave) and 16 v_mov_b32_dpp row_newbcast:i per set, instead of eight
// broadcast 16-byte reads per half (a quarter of the kernel's LDS return bytes); the sets alternate with the halves.
// Measured 0.4 % slower (profiles/r06_dkdv_dpp_ab.txt: LDS return bytes do not limit the kernel, the 32 movs cost
// VALU issue), so it stays off; parity-tested on the GPU all the same
// Timing probes as LCI_FWD_PROBE (variant builds only; results are wrong): bit 0 drops the per-tile barrier, bit 1 the
// wait for tile t+1's staging loads
#ifndef LCI_DKDV_PROBE
#define LCI_DKDV_PROBE 0
#endif
#ifndef LCI_DKDV_DPPRC
#define LCI_DKDV_DPPRC 0
#endif
template <int I>
__device__ __forceinline__ float hs_bcast(float x) {   // lane I of each 16-lane row, to the whole row
  float d;
  asm volatile("v_mov_b32_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(x), "i"(I));
  return d;
}
__device__ __forceinline__ float hs_bcast_i(float x, int i) {   // (i compile-time after unrolling)
  switch (i & 15) {
    case 0: return hs_bcast<0>(x); case 1: return hs_bcast<1>(x); case 2: return hs_bcast<2>(x);
    case 3: return hs_bcast<3>(x); case 4: return hs_bcast<4>(x); case 5: return hs_bcast<5>(x);
    case 6: return hs_bcast<6>(x); case 7: return hs_bcast<7>(x); case 8: return hs_bcast<8>(x);
    case 9: return hs_bcast<9>(x); case 10: return hs_bcast<10>(x); case 11: return hs_bcast<11>(x);
    case 12: return hs_bcast<12>(x); case 13: return hs_bcast<13>(x); case 14: return hs_bcast<14>(x);
    default: return hs_bcast<15>(x);
  }
}
__global__ __launch_bounds__(HS_NW * 64, 1) void attn_bwd_dkdv_hs_kernel(AttnArgs a) {
  constexpr bool DPPRC = LCI_DKDV_DPPRC != 0;
  // the Q | dO ring: tile t, t+1 (published), t+2, t+3 (in flight); the row-constant rows follow in their own 2 KB
  constexpr int RC_B = 2 * KT * 4;                  // -lse2[64] | -delta[64] of one tile
  constexpr int NOPS = 5;                           // LDS-DMA operations per wave and tile (prologue)
  __shared__ __attribute__((aligned(16))) char smem[HS_NSLOT * HS_SLOT_B + HS_NSLOT * RC_B];
  char* const rcs = smem + HS_NSLOT * HS_SLOT_B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = blockIdx.y, b = blockIdx.z;
  const int L = a.L;
  const int h = lane >> 5, r32 = lane & 31;
  const int kw0 = a.k0 + blockIdx.x * (HS_NW * 64) + wave * 64;
  const int nqt = (L + KT - 1) / KT;

  // K^T / V^T as B operands: lane holds K[kw0 + 32kb + r32][16ks + 8h + j] (K prescaled into the exp2 domain)
  bf16x8 kf[2][4], vf[2][4];
  {
    const bf16* kp = a.k + b * a.bs_k + hh * a.hs;
    const bf16* vp = a.v + b * a.bs_v + hh * a.hs;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      hs_load_b2(kf[kb], vf[kb], kp, a.rs_k, vp, a.rs_v, kw0 + 32 * kb + r32, L, h, a.c);
    }
  }
  // the K / V loads complete here: otherwise the compiler waits for them (vmcnt(0)) at their first use inside the
  // loop, where that wait would also drain every tile's in-flight staging loads (which it does not track)
  hs_vmcnt<0>();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      { HS_TO_AGPR(kf[i][j]); HS_TO_AGPR(vf[i][j]); }

  // ---- prologue staging by LDS-DMA: the wave's pieces of the Q and dO tiles (HsRing), and one row of row
  // constants (waves 0 / 2: -lse2, 1 / 3: -delta; the pairs write the same bytes). Rows >= L read as zero: they add
  // nothing to dV or dK whatever P is.
  const int rs2q = a.rs_q * 2, rs2d = a.rs_do * 2;
  const rsrc_t rq = hs_rows_rsrc(a.q + b * a.bs_q + hh * a.hs, rs2q, L);
  const rsrc_t rd = hs_rows_rsrc(a.dout + b * a.bs_do + hh * a.hs, rs2d, L);
  const rsrc_t rr = make_rsrc(a.delta + ((long long)b * a.H + hh) * 2 * L + (wave & 1) * L, (uint32_t)L * 4);
  const HsRing ring = hs_ring(rq, rs2q, rd, rs2d, lane, wave, smem);
  const unsigned lds0 = ring.lds0;
  auto dma_op = [&](int t, int i) __attribute__((always_inline)) {   // operation i (0-4) of tile t
    if (i < 4) ring.dma(t, i);
    if (i == 4) hs_dma4(rr, lane * 4, t * KT * 4,
                        lds0 + (unsigned)(HS_NSLOT * HS_SLOT_B + (t & (HS_NSLOT - 1)) * RC_B + (wave & 1) * KT * 4));
  };
  auto dma_tile = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NOPS; ++i) dma_op(t, i);
  };
  // ---- fragment readers. sw128's swizzle depends on row bits 1-3 only, so a row offset that is a multiple of 16
  // (r0, 16 S) is a plain byte offset: the lane part of every read address is one of 9 registers computed here and
  // kept opaque, and slot (compile-time in the unrolled loop), dO, row and row-constant offsets are DS immediates
  unsigned q_off[4], t_off[2][2], rc_off;   // [k-step] | [d block][part] | row constants: + 16 h
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    q_off[ks] = 2 * sw128(r32, 16 * ks + 8 * h);
    HS_OPAQUE(q_off[ks]);
  }
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int part = 0; part < 2; ++part) {
      t_off[db][part] = 2 * sw128(4 * h + ((lane & 15) >> 2) + 8 * part, 32 * db + 16 * ((lane >> 4) & 1) + 4 * (lane & 3));
      HS_OPAQUE(t_off[db][part]);
    }
  rc_off = HS_NSLOT * HS_SLOT_B + 16 * h;   // (past the 64-KB ring: in the register, the rest is an immediate)
  HS_OPAQUE(rc_off);
  // DPPRC: lane l reads the constant of query (l & 3) + 8 ((l >> 2) & 3) + 4h, register l & 15's row
  unsigned rcx_off = HS_NSLOT * HS_SLOT_B + 4 * ((lane & 3) + 8 * ((lane >> 2) & 3) + 4 * h);
  HS_OPAQUE(rcx_off);
  // soff: byte offset of the tile in the ring (slot, + HS_TILE_B for dO); r0: the half's first query row in the tile
  auto qrow = [&](int soff, int r0, int ks) __attribute__((always_inline)) {
    return *(const bf16x8*)(smem + q_off[ks] + (soff + 2 * DH * r0));
  };
  auto trf = [&](int soff, int r0, int S, int db) __attribute__((always_inline)) {
    const int imm = soff + 2 * DH * (r0 + 16 * S);
    return cat44(lds_tr4((const bf16*)(smem + t_off[db][0] + imm)), lds_tr4((const bf16*)(smem + t_off[db][1] + imm)));
  };
  // initial accumulator of a chain: register i <-> query r0 + (i & 3) + 8 (i >> 2) + 4h
  auto rcblk = [&](const char* rcslot, int which, int r0) __attribute__((always_inline)) {
    const float* rc = (const float*)(rcslot + which * KT * 4) + r0 + 4 * h;
    f32x16 r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *(const f32x4*)(rc + 8 * g);
      r[4 * g] = v[0]; r[4 * g + 1] = v[1]; r[4 * g + 2] = v[2]; r[4 * g + 3] = v[3];
    }
    return r;
  };

  f32x16 dv[2][2], dk[2][2];   // [d block][key block]: dV^T / dK^T, lane = key, rows d = 32db + (i&3) + 8(i>>2) + 4h
  f32x16 S[2], P[2];           // [key block]: S~ - lse2 and dP - delta of the block's current half
  f32x16 NLs[2], NDs[2];       // row constants (-lse2, -delta) of the chains' half ([half parity] with DPPRC, else [0])
  float xNL = 0.f, xND = 0.f;  // DPPRC: the next half's constants, one per lane
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    S[i] = P[i] = f32x16{};
#pragma unroll
    for (int j = 0; j < 2; ++j) dv[i][j] = dk[i][j] = f32x16{};
  }
  u32x4 pk[2][2] = {}, dd[2][2] = {};    // [key block][k-step] bf16 P / dS packs (dword j = elements 2j, 2j+1)
  bf16x8 tdo[2][2][2] = {}, tq[2][2][2] = {};  // [set][d block][k-step] transposed dO / Q fragments: half p uses
                                              // set p & 1 (its kb1 products run in half p+1, beside p+1's reads)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    HS_OPAQUE(S[i]);
    HS_OPAQUE(P[i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      HS_TO_AGPR(dv[i][j]);
      HS_TO_AGPR(dk[i][j]);
      HS_OPAQUE(pk[i][j]);
      HS_OPAQUE(dd[i][j]);
#pragma unroll
      for (int k = 0; k < 2; ++k) { HS_OPAQUE(tdo[i][j][k]); HS_OPAQUE(tq[i][j][k]); }
    }
  }
  bf16x8 qa[4], da[4];                   // Q / dO row fragments of the chains' half

  // VALU of gap g of a segment over elements 8e..8e+7 of key block kb: one exp2, one multiply, one conversion per
  // gap (8 + 4 + 4 issue cycles beside the MFMA's 8 of 32); gaps 0-2 finish the previous segment's block
  // (pkb, pe): its last two multiplies and three conversions
  auto valu_gap = [&](int g, int kb, int e, int pkb, int pe) __attribute__((always_inline)) {
    f32x16& s = S[kb];
    f32x16& p = P[kb];
    const int o = 8 * e, po = 8 * pe;
    HS_EXP(s[o + g]);
    if (g >= 2) HS_MUL(p[o + g - 2], s[o + g - 2]);
    if (g == 0) HS_MUL(P[pkb][po + 6], S[pkb][po + 6]);
    if (g == 1) HS_MUL(P[pkb][po + 7], S[pkb][po + 7]);
    switch (g) {
      case 0: HS_CVT(pk[pkb][pe][3], S[pkb][po + 6], S[pkb][po + 7]); break;
      case 1: HS_CVT(dd[pkb][pe][2], P[pkb][po + 4], P[pkb][po + 5]); break;
      case 2: HS_CVT(dd[pkb][pe][3], P[pkb][po + 6], P[pkb][po + 7]); break;
      case 3: HS_CVT(pk[kb][e][0], s[o], s[o + 1]); break;
      case 4: HS_CVT(pk[kb][e][1], s[o + 2], s[o + 3]); break;
      case 5: HS_CVT(dd[kb][e][0], p[o], p[o + 1]); break;
      case 6: HS_CVT(pk[kb][e][2], s[o + 4], s[o + 5]); break;
      default: HS_CVT(dd[kb][e][1], p[o + 2], p[o + 3]); break;
    }
  };
  // MFMA of gap g of a chain segment (S chain at gaps 0-3, dP chain at gaps 4-7) for key block kb
  auto chain_gap = [&](int g, int kb, int st) __attribute__((always_inline)) {
    if (g == 0) HS_MFMA_C0(S[kb], qa[0], kf[kb][0], NLs[st]);
    else if (g < 4) HS_MFMA_C(S[kb], qa[g], kf[kb][g]);
    else if (g == 4) HS_MFMA_C0(P[kb], da[0], vf[kb][0], NDs[st]);
    else HS_MFMA_C(P[kb], da[g - 4], vf[kb][g - 4]);
  };
  // MFMA of gap g of a gradient segment for key block kb with fragment set st: (k-step s2, d block db, dV | dK)
  auto grad_gap = [&](int g, int kb, int st) __attribute__((always_inline)) {
    const int s2 = g >> 2, db = (g >> 1) & 1;
    const bf16x8 pb = __builtin_bit_cast(bf16x8, pk[kb][s2]);
    const bf16x8 db8 = __builtin_bit_cast(bf16x8, dd[kb][s2]);
    if (g & 1) HS_MFMA_G(dk[db][kb], tq[st][db][s2], db8);
    else HS_MFMA_G(dv[db][kb], tdo[st][db][s2], pb);
  };
  // transposed fragment f (gradient order: k-step f >> 2, d block (f >> 1) & 1, dO^T | Q^T) of rows r0 into set st
  auto tr_load = [&](int f, int st, int soff, int r0) __attribute__((always_inline)) {
    const int s2 = f >> 2, db = (f >> 1) & 1;
    if (f & 1) tq[st][db][s2] = trf(soff, r0, s2, db);
    else tdo[st][db][s2] = trf(soff + HS_TILE_B, r0, s2, db);
  };
  // one f32x4 piece (queries 8g + 4h .. + 3 of the half) of a chain's row-constant block; rcoff: the tile's
  // row-constant slot, bytes from the end of the ring
  auto rc_load = [&](f32x16& r, int rcoff, int which, int r0, int g) __attribute__((always_inline)) {
    const f32x4 v = *(const f32x4*)(smem + rc_off + (rcoff + which * KT * 4 + 4 * (r0 + 8 * g)));
    r[4 * g] = v[0]; r[4 * g + 1] = v[1]; r[4 * g + 2] = v[2]; r[4 * g + 3] = v[3];
  };
  // DPPRC: one lane-mapped constant per lane, and mov k (0-31: -lse2 registers 0-15, then -delta's) of set st
  auto rcx_load = [&](int rcoff, int which, int r0) __attribute__((always_inline)) {
    return *(const float*)(smem + rcx_off + (rcoff + which * KT * 4 + 4 * r0));
  };
  auto bc_mov = [&](int k, int st) __attribute__((always_inline)) {
    if (k < 16) NLs[st][k] = hs_bcast_i(xNL, k);
    else NDs[st][k - 16] = hs_bcast_i(xND, k - 16);
  };
  // the 32 movs over the 19 gaps seg B 5-7, seg C 0-7, seg D 0-7 (j = 0-18): two per gap for j < 13, then one
  // (<= 2 x 4 issue cycles beside the gap's 16 of exp2 / multiply / conversion)
  auto bc_gap = [&](int j, int st) __attribute__((always_inline)) {
    if (j < 13) { bc_mov(2 * j, st); bc_mov(2 * j + 1, st); }
    else bc_mov(13 + j, st);
  };

  // One half-tile p = rows r0 of `slot` (fragment set C = p & 1); segs C / D read half p+1 = rows nr0 of `nslot`.
  // LDS reads, one per gap, each placed at least two gaps after the last MFMA read of the registers it refills
  // (seven wait states for a row-constant block read as an MFMA C operand):
  //   seg A, B: this half's transposed fragments into set C (set C^1 is still read by seg B's kb1 products)
  //   seg C: Q rows of half p+1 (gaps 2-5), -lse2 pieces 0-1 and dO rows 0-1 (gaps 6-7)
  //   seg D: -lse2 pieces 2-3, -delta pieces 0-3, dO rows 2-3
  auto half = [&](auto CUR, int slot, int r0, int nslot, int nrc, int nr0, auto mid, auto sgap)
      __attribute__((always_inline)) {
    constexpr int C = decltype(CUR)::value;
    constexpr int ST = DPPRC ? C : 0, NST = DPPRC ? C ^ 1 : 0;   // row-constant sets of this / the next half
    // seg A: chains kb0 || VALU kb1 (p-1) elements 8-15 (finishing its elements 0-7)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      chain_gap(g, 0, ST);
      valu_gap(g, 1, 1, 1, 0);
      if (!(g & 1)) tr_load(g >> 1, C, slot, r0);
      sgap(0, g);
    }
    mid();
    // seg B: dV / dK kb1 (p-1, set C^1) || VALU kb0 elements 0-7 (finishing kb1 8-15)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      grad_gap(g, 1, C ^ 1);
      valu_gap(g, 0, 0, 1, 1);
      if (!(g & 1)) tr_load(4 + (g >> 1), C, slot, r0);
      if (DPPRC) {   // the next half's rows are readable here (half 1: published by mid()'s barrier)
        if (g == 1) xNL = rcx_load(nrc, 0, nr0);
        if (g == 3) xND = rcx_load(nrc, 1, nr0);
        if (g >= 5) bc_gap(g - 5, NST);
      }
      sgap(1, g);
    }
    // seg C: chains kb1 || VALU kb0 elements 8-15
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      chain_gap(g, 1, ST);
      valu_gap(g, 0, 1, 0, 0);
      if (g == 2) HS_KEEP(NLs[ST]);
      if (g == 6) HS_KEEP(NDs[ST]);
      if (DPPRC) bc_gap(3 + g, NST);
      if (g >= 2 && g < 6) qa[g - 2] = qrow(nslot, nr0, g - 2);
      if (g >= 6) {
        if (!DPPRC) rc_load(NLs[0], nrc, 0, nr0, g - 6);
        da[g - 6] = qrow(nslot + HS_TILE_B, nr0, g - 6);
      }
      sgap(2, g);
    }
    // seg D: dV / dK kb0 (set C) || VALU kb1 elements 0-7 (finishing kb0 8-15)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      grad_gap(g, 0, C);
      valu_gap(g, 1, 0, 0, 1);
      if (DPPRC) bc_gap(11 + g, NST);
      if (g < 2) { if (!DPPRC) rc_load(NLs[0], nrc, 0, nr0, g + 2); }
      else if (g < 6) { if (!DPPRC) rc_load(NDs[0], nrc, 1, nr0, g - 2); }
      else da[g - 4] = qrow(nslot + HS_TILE_B, nr0, g - 4);
      sgap(3, g);
    }
  };

  // register staging (as the forward / dQ): tile t+1's Q / dO pieces and row constants (loaded into
  // AGPRs during tile t-1) are stored at seg A gaps 1-7 / seg B gap 1 of tile t's half 0, tile t+2's loaded at seg C
  // gaps 1-7 / seg D gap 1; half 1's barrier publishes tile t+1
  u32x4 rsq[4];
  uint32_t rsr = 0;
  const unsigned wst = lds0 + 2048 * wave + 16 * lane;
  // (past the ring: in the register)
  const unsigned wrc = lds0 + HS_NSLOT * HS_SLOT_B + (wave & 1) * KT * 4 + 4 * lane;
  auto ld_piece = [&](int t, int i) __attribute__((always_inline)) {
    if (i < 4) rsq[i] = hs_ld16(ring.rsrc(i), ring.voff(i), ring.soff(t, i));
    if (i == 4) rsr = hs_ld4(rr, lane * 4, t * KT * 4);
  };
  // prologue: tile 0 by LDS-DMA, tile 1 into the staging registers (5 memory operations per wave and tile)
  dma_tile(0);
  ld_piece(1, 0); ld_piece(1, 1); ld_piece(1, 2); ld_piece(1, 3); ld_piece(1, 4);
  hs_vmcnt<0>();
  __syncthreads();
  NLs[0] = rcblk(rcs, 0, 0);
  NDs[0] = rcblk(rcs, 1, 0);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qa[ks] = qrow(0, 0, ks);
    da[ks] = qrow(HS_TILE_B, 0, ks);
  }
  // the prologue's reads complete here (a waitcnt the compiler's pass sees): otherwise its wait for them, merged
  // into the loop header with the back edge's, makes every tile start with lgkmcnt(1)
  __builtin_amdgcn_s_waitcnt(LGKM0_WAIT);
  // one tile in ring slot SL (compile-time in the 4-tile unroll: every fragment read is a DS immediate off one of
  // the lane registers above) or, SL < 0, t & 3 at run time
  auto tile = [&](auto SL, int t) __attribute__((always_inline)) {
    constexpr int SLC = decltype(SL)::value;
    const int sl = SLC >= 0 ? SLC : t & (HS_NSLOT - 1);
    const int nsl = SLC >= 0 ? (SLC + 1) & (HS_NSLOT - 1) : (t + 1) & (HS_NSLOT - 1);
    const int slot = sl * HS_SLOT_B, nslot = nsl * HS_SLOT_B, rc = sl * RC_B, nrc = nsl * RC_B;
    // tile t+1 (stored from registers in half 0) is published after seg A of half 1 (seg C of half 1 is its first
    // reader): one barrier; no LDS fence: the stores were ordered by the waits of this wave's own later reads
    auto stage = [&]() __attribute__((always_inline)) {
      if (!(LCI_DKDV_PROBE & 1) && t + 1 < nqt) __builtin_amdgcn_s_barrier();
    };
    // half 0: tile t+1's pieces (loaded a tile ago) stored at seg A gaps 1-7 and seg B gap 1... (SS = 0), tile t+2's
    // loaded at seg C gaps 1-7 (LS = 2)
    auto rstg0 = [&](int seg, int g) __attribute__((always_inline)) {
      if (!(g & 1)) return;
      constexpr int SS = 0, LS = 2;   // store / load segments of half 0
      if (!(LCI_DKDV_PROBE & 2) && seg == SS && g == 1) hs_vmcnt<0>();   // tile t+1's pieces (loaded a tile ago)
      constexpr int S1 = SLC >= 0 ? ((SLC + 1) & (HS_NSLOT - 1)) * HS_SLOT_B : 0;
      constexpr int R1 = SLC >= 0 ? ((SLC + 1) & (HS_NSLOT - 1)) * RC_B : 0;
      const unsigned base = SLC >= 0 ? wst : wst + (unsigned)nslot;
      const unsigned rbase = SLC >= 0 ? wrc : wrc + (unsigned)nrc;
      if (seg == SS) {
        switch (g) {
          case 1: hs_st16<S1>(base, rsq[0]); break;
          case 3: hs_st16<S1 + 1024>(base, rsq[1]); break;
          case 5: hs_st16<S1 + HS_TILE_B>(base, rsq[2]); break;
          default: hs_st16<S1 + HS_TILE_B + 1024>(base, rsq[3]); hs_st4<R1>(rbase, rsr); break;
        }
      }
      if (seg == LS) {
        ld_piece(t + 2, g >> 1);
        if (g == 7) ld_piece(t + 2, 4);
      }
    };
    auto none = []() __attribute__((always_inline)) {};
    auto nogap = [](int, int) __attribute__((always_inline)) {};
    half(std::integral_constant<int, 0>{}, slot, 0, slot, rc, 32, none, rstg0);    // segs C / D: rows 32-63
    half(std::integral_constant<int, 1>{}, slot, 32, nslot, nrc, 0, stage, nogap); // ... tile t+1's rows 0-31
  };
  int t = 0;
  for (; t + 4 <= nqt; t += 4) {   // t & 3 == 0 here
    tile(std::integral_constant<int, 0>{}, t);
    tile(std::integral_constant<int, 1>{}, t + 1);
    tile(std::integral_constant<int, 2>{}, t + 2);
    tile(std::integral_constant<int, 3>{}, t + 3);
  }
  for (; t < nqt; ++t) tile(std::integral_constant<int, -1>{}, t);
  hs_vmcnt<0>();   // the last tiles' staging loads (past the end: zeros) retire
  // key block 1 of the last half: elements 8-15 (finishing 0-7), then its dV / dK
#pragma unroll
  for (int g = 0; g < 8; ++g) valu_gap(g, 1, 1, 1, 0);
  HS_MUL(P[1][14], S[1][14]);
  HS_MUL(P[1][15], S[1][15]);
  asm volatile("s_nop 0" ::: "memory");
  HS_CVT(pk[1][1][3], S[1][14], S[1][15]);
  HS_CVT(dd[1][1][2], P[1][12], P[1][13]);
  HS_CVT(dd[1][1][3], P[1][14], P[1][15]);
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int g = 0; g < 8; ++g) grad_gap(g, 1, 1);   // the last half is a half 1 (set 1)
  // the accumulators are read by VALU next: let the last MFMAs retire (the compiler cannot see their latency)
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");

  const float sc = a.scale;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const int key = kw0 + 32 * kb + r32;
    if (key < L) {
      bf16* dkp = a.dk + b * a.bs_dk + (long long)key * a.rs_dk + hh * a.hs;
      bf16* dvp = a.dv + b * a.bs_dv + (long long)key * a.rs_dv + hh * a.hs;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 k4, v4;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            k4[j] = to_bf16(dk[db][kb][4 * g + j] * sc);
            v4[j] = to_bf16(dv[db][kb][4 * g + j]);
          }
          *(bf16x4*)(dkp + 32 * db + 8 * g + 4 * h) = k4;
          *(bf16x4*)(dvp + 32 * db + 8 * g + 4 * h) = v4;
        }
    }
  }
}

// ------------------------------------------------- backward: dK, dV kernel, 96 keys per wave (three key blocks)
// attn_bwd_dkdv_hs_kernel's stream with a third key block per wave: a workgroup owns 4 x 96 = 384 keys, and every Q /
// dO fragment read from LDS feeds three key blocks. Per 32-query half 48 MFMAs against the narrow kernel's 32 LDS
// reads, staging and barrier: 0.67 LDS reads per MFMA instead of 1. Per key the operations and their order over the
// queries are the narrow kernel's, so dK and dV are bitwise the same.
// Six segments of 8 gaps per half p; block kb's chains, its VALU (two segments) and its products follow each other as
// in the narrow kernel, the three blocks two segments apart:
//   seg A: chains kb0 (p)          || VALU kb2 (p-1) elements 8-15
//   seg B: dV^T / dK^T kb2 (p-1)   || VALU kb0 elements 0-7   | LDS: dO^T / Q^T of half p (gaps 2-7)
//   seg C: chains kb1              || VALU kb0 elements 8-15  | LDS: dO^T / Q^T (gaps 0-1)
//   seg D: dV^T / dK^T kb0         || VALU kb1 elements 0-7
//   seg E: chains kb2              || VALU kb1 elements 8-15  | LDS: Q rows of p+1, -lse2, dO rows (the narrow seg C)
//   seg F: dV^T / dK^T kb1         || VALU kb2 elements 0-7   | LDS: -lse2, -delta, dO rows (the narrow seg D)
// Registers: the 192 accumulators and the K / V fragments of blocks 0 and 1 fill the AGPR half (256); block 2's
// fragments live in the arch half, which has room for them because
//   - only two blocks' S / dP and packs are live at a time: block kb of half p uses set (kb & 1) ^ (p & 1) (block 2
//     takes over block 0's set two segments after block 0's last pack, block 0 of the next half block 1's);
//   - one set of transposed fragments serves all three blocks: fragment f is last read by block 2's products at
//     seg B gap f of the next half and refilled at gap f + 2, four gaps or more before block 0's products read it.
// Ring, prologue, ragged last tile, barrier and the 4-tile unroll are the narrow kernel's; the tiles arrive by LDS-DMA
// (no register is left for staging). Staging reads reach tile nqt + 1: rows below L + 3 KT, inside the bound attn_check
// sets for every placed kernel.
constexpr int DKV3_KWG = HS_NW * 96;   // keys per workgroup
__global__ __launch_bounds__(HS_NW * 64, 1) void attn_bwd_dkdv_hs3_kernel(AttnArgs a) {
  constexpr int RC_B = 2 * KT * 4;                  // -lse2[64] | -delta[64] of one tile
  constexpr int NOPS = 5;                           // LDS-DMA operations per wave and tile (prologue)
  __shared__ __attribute__((aligned(16))) char smem[HS_NSLOT * HS_SLOT_B + HS_NSLOT * RC_B];
  char* const rcs = smem + HS_NSLOT * HS_SLOT_B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = blockIdx.y, b = blockIdx.z;
  const int L = a.L;
  const int h = lane >> 5, r32 = lane & 31;
  const int kw0 = blockIdx.x * DKV3_KWG + wave * 96;
  const int nqt = (L + KT - 1) / KT;

  // K^T / V^T as B operands: lane holds K[kw0 + 32kb + r32][16ks + 8h + j] (K prescaled into the exp2 domain)
  bf16x8 kf[3][4], vf[3][4];
  {
    const bf16* kp = a.k + b * a.bs_k + hh * a.hs;
    const bf16* vp = a.v + b * a.bs_v + hh * a.hs;
#pragma unroll
    for (int kb = 0; kb < 3; ++kb) {
      hs_load_b2(kf[kb], vf[kb], kp, a.rs_k, vp, a.rs_v, kw0 + 32 * kb + r32, L, h, a.c);
    }
  }
  // the K / V loads complete here (as the narrow kernel)
  hs_vmcnt<0>();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    HS_TO_AGPR(kf[0][j]); HS_TO_AGPR(vf[0][j]);
    HS_TO_AGPR(kf[1][j]); HS_TO_AGPR(vf[1][j]);
    HS_OPAQUE(kf[2][j]); HS_OPAQUE(vf[2][j]);
  }

  // ---- prologue staging by LDS-DMA (as the narrow kernel)
  const int rs2q = a.rs_q * 2, rs2d = a.rs_do * 2;
  const rsrc_t rq = hs_rows_rsrc(a.q + b * a.bs_q + hh * a.hs, rs2q, L);
  const rsrc_t rd = hs_rows_rsrc(a.dout + b * a.bs_do + hh * a.hs, rs2d, L);
  const rsrc_t rr = make_rsrc(a.delta + ((long long)b * a.H + hh) * 2 * L + (wave & 1) * L, (uint32_t)L * 4);
  const HsRing ring = hs_ring(rq, rs2q, rd, rs2d, lane, wave, smem);
  const unsigned lds0 = ring.lds0;
  auto dma_op = [&](int t, int i) __attribute__((always_inline)) {   // operation i (0-4) of tile t
    if (i < 4) ring.dma(t, i);
    if (i == 4) hs_dma4(rr, lane * 4, t * KT * 4,
                        lds0 + (unsigned)(HS_NSLOT * HS_SLOT_B + (t & (HS_NSLOT - 1)) * RC_B + (wave & 1) * KT * 4));
  };
  // ---- fragment readers: the narrow kernel's 9 lane registers, everything else a DS immediate
  unsigned q_off[4], t_off[2][2], rc_off;   // [k-step] | [d block][part] | row constants: + 16 h
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    q_off[ks] = 2 * sw128(r32, 16 * ks + 8 * h);
    HS_OPAQUE(q_off[ks]);
  }
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int part = 0; part < 2; ++part) {
      t_off[db][part] = 2 * sw128(4 * h + ((lane & 15) >> 2) + 8 * part, 32 * db + 16 * ((lane >> 4) & 1) + 4 * (lane & 3));
      HS_OPAQUE(t_off[db][part]);
    }
  rc_off = HS_NSLOT * HS_SLOT_B + 16 * h;   // (past the 64-KB ring: in the register, the rest is an immediate)
  HS_OPAQUE(rc_off);
  auto qrow = [&](int soff, int r0, int ks) __attribute__((always_inline)) {
    return *(const bf16x8*)(smem + q_off[ks] + (soff + 2 * DH * r0));
  };
  auto trf = [&](int soff, int r0, int S, int db) __attribute__((always_inline)) {
    const int imm = soff + 2 * DH * (r0 + 16 * S);
    return cat44(lds_tr4((const bf16*)(smem + t_off[db][0] + imm)), lds_tr4((const bf16*)(smem + t_off[db][1] + imm)));
  };
  auto rcblk = [&](const char* rcslot, int which, int r0) __attribute__((always_inline)) {
    const float* rc = (const float*)(rcslot + which * KT * 4) + r0 + 4 * h;
    f32x16 r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *(const f32x4*)(rc + 8 * g);
      r[4 * g] = v[0]; r[4 * g + 1] = v[1]; r[4 * g + 2] = v[2]; r[4 * g + 3] = v[3];
    }
    return r;
  };

  f32x16 dv[2][3], dk[2][3];   // [d block][key block]: dV^T / dK^T, lane = key, rows d = 32db + (i&3) + 8(i>>2) + 4h
  f32x16 S[2], P[2];           // [set]: S~ - lse2 and dP - delta of a block's current half
  f32x16 NLs, NDs;             // row constants (-lse2, -delta) of the chains' half
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    S[i] = P[i] = f32x16{};
#pragma unroll
    for (int j = 0; j < 3; ++j) dv[i][j] = dk[i][j] = f32x16{};
  }
  u32x4 pk[2][2] = {}, dd[2][2] = {};    // [set][k-step] bf16 P / dS packs (dword j = elements 2j, 2j+1)
  bf16x8 tdo[2][2] = {}, tq[2][2] = {};  // [d block][k-step] transposed dO / Q fragments of the products' half
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    HS_OPAQUE(S[i]);
    HS_OPAQUE(P[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      HS_TO_AGPR(dv[i][j]);
      HS_TO_AGPR(dk[i][j]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      HS_OPAQUE(pk[i][j]);
      HS_OPAQUE(dd[i][j]);
      HS_OPAQUE(tdo[i][j]);
      HS_OPAQUE(tq[i][j]);
    }
  }
  bf16x8 qa[4], da[4];                   // Q / dO row fragments of the chains' half

  // VALU of gap g of a segment over elements 8e..8e+7 of set st, finishing set pst's elements 8pe..8pe+7 at gaps 0-2
  // (the narrow kernel's valu_gap)
  auto valu_gap = [&](int g, int st, int e, int pst, int pe) __attribute__((always_inline)) {
    f32x16& s = S[st];
    f32x16& p = P[st];
    const int o = 8 * e, po = 8 * pe;
    HS_EXP(s[o + g]);
    if (g >= 2) HS_MUL(p[o + g - 2], s[o + g - 2]);
    if (g == 0) HS_MUL(P[pst][po + 6], S[pst][po + 6]);
    if (g == 1) HS_MUL(P[pst][po + 7], S[pst][po + 7]);
    switch (g) {
      case 0: HS_CVT(pk[pst][pe][3], S[pst][po + 6], S[pst][po + 7]); break;
      case 1: HS_CVT(dd[pst][pe][2], P[pst][po + 4], P[pst][po + 5]); break;
      case 2: HS_CVT(dd[pst][pe][3], P[pst][po + 6], P[pst][po + 7]); break;
      case 3: HS_CVT(pk[st][e][0], s[o], s[o + 1]); break;
      case 4: HS_CVT(pk[st][e][1], s[o + 2], s[o + 3]); break;
      case 5: HS_CVT(dd[st][e][0], p[o], p[o + 1]); break;
      case 6: HS_CVT(pk[st][e][2], s[o + 4], s[o + 5]); break;
      default: HS_CVT(dd[st][e][1], p[o + 2], p[o + 3]); break;
    }
  };
  // MFMA of gap g of a chain segment (S chain at gaps 0-3, dP chain at gaps 4-7) for key block kb into set st
  auto chain_gap = [&](int g, int kb, int st) __attribute__((always_inline)) {
    if (kb < 2) {
      if (g == 0) HS_MFMA_C0(S[st], qa[0], kf[kb][0], NLs);
      else if (g < 4) HS_MFMA_C(S[st], qa[g], kf[kb][g]);
      else if (g == 4) HS_MFMA_C0(P[st], da[0], vf[kb][0], NDs);
      else HS_MFMA_C(P[st], da[g - 4], vf[kb][g - 4]);
    } else {
      if (g == 0) HS_MFMA_C0V(S[st], qa[0], kf[2][0], NLs);
      else if (g < 4) HS_MFMA_CV(S[st], qa[g], kf[2][g]);
      else if (g == 4) HS_MFMA_C0V(P[st], da[0], vf[2][0], NDs);
      else HS_MFMA_CV(P[st], da[g - 4], vf[2][g - 4]);
    }
  };
  // MFMA of gap g of a gradient segment for key block kb with pack set st: (k-step s2, d block db, dV | dK)
  auto grad_gap = [&](int g, int kb, int st) __attribute__((always_inline)) {
    const int s2 = g >> 2, db = (g >> 1) & 1;
    const bf16x8 pb = __builtin_bit_cast(bf16x8, pk[st][s2]);
    const bf16x8 db8 = __builtin_bit_cast(bf16x8, dd[st][s2]);
    if (g & 1) HS_MFMA_G(dk[db][kb], tq[db][s2], db8);
    else HS_MFMA_G(dv[db][kb], tdo[db][s2], pb);
  };
  // transposed fragment f (gradient order: k-step f >> 2, d block (f >> 1) & 1, dO^T | Q^T) of rows r0: the
  // operand of gap f of every gradient segment
  auto tr_load = [&](int f, int soff, int r0) __attribute__((always_inline)) {
    const int s2 = f >> 2, db = (f >> 1) & 1;
    if (f & 1) tq[db][s2] = trf(soff, r0, s2, db);
    else tdo[db][s2] = trf(soff + HS_TILE_B, r0, s2, db);
  };
  auto rc_load = [&](f32x16& r, int rcoff, int which, int r0, int g) __attribute__((always_inline)) {
    const f32x4 v = *(const f32x4*)(smem + rc_off + (rcoff + which * KT * 4 + 4 * (r0 + 8 * g)));
    r[4 * g] = v[0]; r[4 * g + 1] = v[1]; r[4 * g + 2] = v[2]; r[4 * g + 3] = v[3];
  };

  // One half-tile p = rows r0 of `slot`, parity C; segs E / F read half p+1 = rows nr0 of `nslot`. LDS reads one per
  // gap (two at seg E gaps 6-7), each at least two gaps after the last MFMA read of the registers it refills (seven
  // wait states for a row-constant block read as an MFMA C operand).
  auto half = [&](auto CUR, int slot, int r0, int nslot, int nrc, int nr0, auto mid, auto sgap)
      __attribute__((always_inline)) {
    constexpr int X = decltype(CUR)::value, Y = X ^ 1;   // sets of blocks 0, 2 | of block 1 and of block 2 of half p-1
    // seg A: chains kb0 || VALU kb2 (p-1) elements 8-15 (finishing its elements 0-7)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      chain_gap(g, 0, X);
      valu_gap(g, Y, 1, Y, 0);
      sgap(0, g);
    }
    mid();
    // seg B: dV / dK kb2 (p-1) || VALU kb0 elements 0-7 (finishing kb2 8-15)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      grad_gap(g, 2, Y);
      valu_gap(g, X, 0, Y, 1);
      if (g >= 2) tr_load(g - 2, slot, r0);
      sgap(1, g);
    }
    // seg C: chains kb1 || VALU kb0 elements 8-15
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      chain_gap(g, 1, Y);
      valu_gap(g, X, 1, X, 0);
      if (g < 2) tr_load(6 + g, slot, r0);
      sgap(2, g);
    }
    // seg D: dV / dK kb0 || VALU kb1 elements 0-7 (finishing kb0 8-15)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      grad_gap(g, 0, X);
      valu_gap(g, Y, 0, X, 1);
      sgap(3, g);
    }
    // seg E: chains kb2 (block 0's set) || VALU kb1 elements 8-15
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      chain_gap(g, 2, X);
      valu_gap(g, Y, 1, Y, 0);
      if (g == 2) HS_KEEP(NLs);
      if (g == 6) HS_KEEP(NDs);
      if (g >= 2 && g < 6) qa[g - 2] = qrow(nslot, nr0, g - 2);
      if (g >= 6) {
        rc_load(NLs, nrc, 0, nr0, g - 6);
        da[g - 6] = qrow(nslot + HS_TILE_B, nr0, g - 6);
      }
      sgap(4, g);
    }
    // seg F: dV / dK kb1 || VALU kb2 elements 0-7 (finishing kb1 8-15)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      grad_gap(g, 1, Y);
      valu_gap(g, X, 0, Y, 1);
      if (g < 2) rc_load(NLs, nrc, 0, nr0, g + 2);
      else if (g < 6) rc_load(NDs, nrc, 1, nr0, g - 2);
      else da[g - 4] = qrow(nslot + HS_TILE_B, nr0, g - 4);
      sgap(5, g);
    }
  };

  // staging by LDS-DMA straight into the ring (the arch half has no room for staging registers): tile t+2's five
  // pieces are issued at seg C gaps 1-7 of tile t's half 0. Its slot held tile t-2, which every wave finished reading
  // before tile t-1's barrier. Tile t+1's barrier waits for all but the wave's five youngest operations (tile t+3's,
  // issued in its half 0) and publishes tile t+2 for seg E of its half 1.
  // prologue: tiles 0 and 1
#pragma unroll
  for (int i = 0; i < NOPS; ++i) dma_op(0, i);
#pragma unroll
  for (int i = 0; i < NOPS; ++i) dma_op(1, i);
  hs_vmcnt<0>();
  __syncthreads();
  NLs = rcblk(rcs, 0, 0);
  NDs = rcblk(rcs, 1, 0);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qa[ks] = qrow(0, 0, ks);
    da[ks] = qrow(HS_TILE_B, 0, ks);
  }
  // the prologue's reads complete here (as the narrow kernel)
  __builtin_amdgcn_s_waitcnt(LGKM0_WAIT);
  // one tile in ring slot SL (compile-time in the 4-tile unroll) or, SL < 0, t & 3 at run time
  auto tile = [&](auto SL, int t) __attribute__((always_inline)) {
    constexpr int SLC = decltype(SL)::value;
    const int sl = SLC >= 0 ? SLC : t & (HS_NSLOT - 1);
    const int nsl = SLC >= 0 ? (SLC + 1) & (HS_NSLOT - 1) : (t + 1) & (HS_NSLOT - 1);
    const int slot = sl * HS_SLOT_B, nslot = nsl * HS_SLOT_B, nrc = nsl * RC_B;
    // tile t+1 is published after seg A of half 1 (seg E of half 1 is its first reader): one barrier behind the
    // counted wait for its pieces
    auto stage = [&]() __attribute__((always_inline)) {
      if (t + 1 < nqt) {
        hs_vmcnt<NOPS>();
        __builtin_amdgcn_s_barrier();
      }
    };
    auto rstg0 = [&](int seg, int g) __attribute__((always_inline)) {
      if (seg != 2 || !(g & 1)) return;
      dma_op(t + 2, g >> 1);
      if (g == 7) dma_op(t + 2, 4);
    };
    auto none = []() __attribute__((always_inline)) {};
    auto nogap = [](int, int) __attribute__((always_inline)) {};
    half(std::integral_constant<int, 0>{}, slot, 0, slot, sl * RC_B, 32, none, rstg0);   // segs E / F: rows 32-63
    half(std::integral_constant<int, 1>{}, slot, 32, nslot, nrc, 0, stage, nogap);       // ... tile t+1's rows 0-31
  };
  int t = 0;
  for (; t + 4 <= nqt; t += 4) {   // t & 3 == 0 here
    tile(std::integral_constant<int, 0>{}, t);
    tile(std::integral_constant<int, 1>{}, t + 1);
    tile(std::integral_constant<int, 2>{}, t + 2);
    tile(std::integral_constant<int, 3>{}, t + 3);
  }
  for (; t < nqt; ++t) tile(std::integral_constant<int, -1>{}, t);
  hs_vmcnt<0>();   // the last tiles' staging loads (past the end: zeros) retire
  // key block 2 of the last half (a half 1: set 1): elements 8-15 (finishing 0-7), then its dV / dK
#pragma unroll
  for (int g = 0; g < 8; ++g) valu_gap(g, 1, 1, 1, 0);
  HS_MUL(P[1][14], S[1][14]);
  HS_MUL(P[1][15], S[1][15]);
  asm volatile("s_nop 0" ::: "memory");
  HS_CVT(pk[1][1][3], S[1][14], S[1][15]);
  HS_CVT(dd[1][1][2], P[1][12], P[1][13]);
  HS_CVT(dd[1][1][3], P[1][14], P[1][15]);
  asm volatile("s_nop 1" ::: "memory");
#pragma unroll
  for (int g = 0; g < 8; ++g) grad_gap(g, 2, 1);
  // the accumulators are read by VALU next: let the last MFMAs retire (the compiler cannot see their latency)
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");

  // the lane's key and column are derived again from the thread index, made opaque: one register lives across the
  // loop for the stores, not every value derived from it
  int etid = tid;
  HS_OPAQUE(etid);
  const int eh = (etid >> 5) & 1, er32 = etid & 31;
  const float sc = a.scale;
#pragma unroll
  for (int kb = 0; kb < 3; ++kb) {
    const int key = kw0 + 32 * kb + er32;
    if (key < L) {
      bf16* dkp = a.dk + b * a.bs_dk + (long long)key * a.rs_dk + hh * a.hs;
      bf16* dvp = a.dv + b * a.bs_dv + (long long)key * a.rs_dv + hh * a.hs;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 k4, v4;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            k4[j] = to_bf16(dk[db][kb][4 * g + j] * sc);
            v4[j] = to_bf16(dv[db][kb][4 * g + j]);
          }
          *(bf16x4*)(dkp + 32 * db + 8 * g + 4 * eh) = k4;
          *(bf16x4*)(dvp + 32 * db + 8 * g + 4 * eh) = v4;
        }
    }
  }
}

// --------------------------------------- backward: dQ kernel, one wave per SIMD, placed MFMA / VALU / LDS stream
// The dK/dV kernel's structure for dQ (query on the MFMA lane): a workgroup = 4 waves, a wave owns 64 queries (two
// query blocks of 32, Q~ / dO fragments in AGPRs, -lse2 / -delta splats as the chains' initial accumulators, dQ^T in
// AGPRs), key tiles of 64 keys (K, V; 128-B sw128 rows) arrive in a 4-slot ring, staged through AGPRs one tile
// ahead (buffer loads during tile t-1, ds_write during tile t's half 0).
// Per 32-key half-tile and wave: 24 MFMAs (S^T = K Q~^T and dP^T = V dO^T chains, 4 + 4 per query block;
// dQ^T += K^T dS^T, 4 per block) against 32 exp2 + 32 multiplies + 16 conversions. MFMA order per half:
//   gaps 0-7: chains of block 0 | 8-11: dQ^T of block 1 (previous half) | 12-19: chains of block 1 |
//   20-23: dQ^T of block 0,
// the VALU of each gap from DQ_SCHED (tools/gen_dq_sched.py: <= 2 exp2 and <= 4 VALU per gap, every dependency
// distance and pack deadline checked); LDS reads one per gap: V rows of this half at gaps 0-3, the transposed K
// fragments (dQ^T's A operand, shared by both blocks) at 12-19, K rows of the next half at 20-23.
// Keys past L read as zero rows (dS^T there multiplies zero K); no masking.
// gap  0: E1.8 E1.9
// gap  1: M1.8 M1.9 E1.10 C1.4
// gap  2: M1.10 E1.11 E1.12
// gap  3: M1.11 M1.12 C1.5 E1.13
// gap  4: E1.14 M1.13 E1.15 C1.6
// gap  5: M1.14 M1.15 E0.0 C1.7
// gap  6: E0.1 E0.2
// gap  7: E0.3 E0.4
// gap  8: E0.5 E0.6
// gap  9: M0.0 M0.1 M0.2 M0.3
// gap 10: C0.0 C0.1 M0.4 M0.5
// gap 11: M0.6 C0.2 E0.7 E0.8
// gap 12: M0.7 M0.8 C0.3 E0.9
// gap 13: E0.10 M0.9 E0.11 C0.4
// gap 14: M0.10 M0.11 E0.12 C0.5
// gap 15: M0.12 E0.13 E0.14
// gap 16: M0.13 M0.14 C0.6 E0.15
// gap 17: E1.0 M0.15 E1.1 C0.7
// gap 18: E1.2 E1.3
// gap 19: E1.4 E1.5
// gap 20: E1.6 E1.7
// gap 21: M1.0 M1.1 M1.2 M1.3
// gap 22: C1.0 C1.1 M1.4 M1.5
// gap 23: M1.6 M1.7 C1.2 C1.3
constexpr unsigned char DQ_SCHED[24][4] = {
    {0x28, 0x29, 0xff, 0xff},
    {0x68, 0x69, 0x2a, 0xa4},
    {0x6a, 0x2b, 0x2c, 0xff},
    {0x6b, 0x6c, 0xa5, 0x2d},
    {0x2e, 0x6d, 0x2f, 0xa6},
    {0x6e, 0x6f, 0x00, 0xa7},
    {0x01, 0x02, 0xff, 0xff},
    {0x03, 0x04, 0xff, 0xff},
    {0x05, 0x06, 0xff, 0xff},
    {0x40, 0x41, 0x42, 0x43},
    {0x80, 0x81, 0x44, 0x45},
    {0x46, 0x82, 0x07, 0x08},
    {0x47, 0x48, 0x83, 0x09},
    {0x0a, 0x49, 0x0b, 0x84},
    {0x4a, 0x4b, 0x0c, 0x85},
    {0x4c, 0x0d, 0x0e, 0xff},
    {0x4d, 0x4e, 0x86, 0x0f},
    {0x20, 0x4f, 0x21, 0x87},
    {0x22, 0x23, 0xff, 0xff},
    {0x24, 0x25, 0xff, 0xff},
    {0x26, 0x27, 0xff, 0xff},
    {0x60, 0x61, 0x62, 0x63},
    {0xa0, 0xa1, 0x64, 0x65},
    {0x66, 0x67, 0xa2, 0xa3}};


#ifndef LCI_DQ_EARLY
#define LCI_DQ_EARLY 1
#endif
constexpr bool DQ_EARLY = LCI_DQ_EARLY != 0;
// (the body of attn_bwd_dq_hs_kernel and of attn_bwd_dq_hsfb_kernel, the wide kernel's fallback, below)
__device__ __forceinline__ void attn_bwd_dq_hs_body(const AttnArgs& a) {
  __shared__ __attribute__((aligned(16))) char smem[HS_NSLOT * HS_SLOT_B];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = blockIdx.y, b = blockIdx.z;
  const int L = a.L;
  const int h = lane >> 5, r32 = lane & 31;
  const int qw0 = blockIdx.x * (HS_NW * 64) + wave * 64;
  const int nkt = (L + KT - 1) / KT;
  const int nkt4 = (nkt + 3) & ~3;

  // Q~ / dO as B operands: lane holds X[qw0 + 32qb + r32][16ks + 8h + j] (Q prescaled into the exp2 domain);
  // -lse2 / -delta of the lane's query splatted over a chain's 16 accumulator registers
  bf16x8 qf[2][4], df[2][4];
  f32x16 NL[2], ND[2];
  {
    const bf16* qp = a.q + b * a.bs_q + hh * a.hs;
    const bf16* dop = a.dout + b * a.bs_do + hh * a.hs;
    const float* ws = a.delta + ((long long)b * a.H + hh) * 2 * L;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int q = qw0 + 32 * qb + r32;
      float nl = 0.f, nd = 0.f;
      hs_load_b2(qf[qb], df[qb], qp, a.rs_q, dop, a.rs_do, q, L, h, a.c);
      if (q < L) { nl = ws[q]; nd = ws[L + q]; }
#pragma unroll
      for (int i = 0; i < 16; ++i) { NL[qb][i] = nl; ND[qb][i] = nd; }
    }
  }
  hs_vmcnt<0>();   // (see the dK/dV kernel: no compiler vmcnt wait inside the loop)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      { HS_TO_AGPR(qf[i][j]); HS_TO_AGPR(df[i][j]); }

  // ---- K / V tile pieces (wave w: rows 16w .. 16w+15 of each, 1-KB pieces of 8 rows): tile 0 by LDS-DMA
  const int rs2k = a.rs_k * 2, rs2v = a.rs_v * 2;
  const HsRing ring = hs_ring(hs_rows_rsrc(a.k + b * a.bs_k + hh * a.hs, rs2k, L), rs2k,
                              hs_rows_rsrc(a.v + b * a.bs_v + hh * a.hs, rs2v, L), rs2v, lane, wave, smem);

  // LDS byte offsets of every distinct fragment read within a ring slot, computed once and kept opaque (see the
  // forward kernel): with a compile-time ring slot every read is a lane register + an immediate
  unsigned row_off[2][4], tr_off[2][4][2];   // [rows 0-31 | 32-63][k-step | fragment][part]
#pragma unroll
  for (int r0i = 0; r0i < 2; ++r0i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      row_off[r0i][k] = 2 * sw128(32 * r0i + r32, 16 * k + 8 * h);
      HS_OPAQUE(row_off[r0i][k]);
#pragma unroll
      for (int part = 0; part < 2; ++part) {   // fragment k = (d block k & 1, k-step k >> 1)
        const int rw = 32 * r0i + 16 * (k >> 1) + 4 * h + ((lane & 15) >> 2) + 8 * part;
        const int col = 32 * (k & 1) + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        tr_off[r0i][k][part] = 2 * sw128(rw, col);
        HS_OPAQUE(tr_off[r0i][k][part]);
      }
    }
  auto row = [&](int soff, int r0i, int ks) __attribute__((always_inline)) {   // soff: slot (+ HS_TILE_B for V) bytes
    return *(const bf16x8*)(smem + row_off[r0i][ks] + soff);
  };
  auto trh = [&](int soff, int r0i, int f, int part) __attribute__((always_inline)) {
    return lds_tr4((const bf16*)(smem + tr_off[r0i][f][part] + soff));
  };

  f32x16 dq[2][2];             // [d block][query block]: dQ^T, lane = query, rows d = 32db + (i&3) + 8(i>>2) + 4h
  f32x16 S[2], P[2];           // [query block]: S~^T - lse2, dP^T - delta (rows = the half's 32 keys)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    S[i] = P[i] = f32x16{};
#pragma unroll
    for (int j = 0; j < 2; ++j) dq[i][j] = f32x16{};
  }
  u32x4 dsp[2][2] = {};        // [query block][k-step] bf16 dS^T packs
  // [set][d block][k-step][half of the fragment] transposed K (keys as the k index). Only set 0 is read; set 1 is
  // an opaque dead copy that keeps the register allocation (and so the placed stream) of the measured build
  bf16x4 ktr[2][2][2][2] = {};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    HS_OPAQUE(S[i]);
    HS_OPAQUE(P[i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      HS_TO_AGPR(dq[i][j]);
      HS_OPAQUE(dsp[i][j]);
#pragma unroll
      for (int k = 0; k < 2; ++k) { HS_OPAQUE(ktr[k][i][j][0]); HS_OPAQUE(ktr[k][i][j][1]); }
    }
  }
  bf16x8 kr[4], vr[4];         // K / V row fragments (A operands of the chains)

  auto valu_op = [&](unsigned char c, int only_qb) __attribute__((always_inline)) {
    if (c == 0xFF) return;
    const int kind = c >> 6, qb = (c >> 5) & 1, i = c & 31;
    if (only_qb >= 0 && qb != only_qb) return;
    if (kind == 0) HS_EXP(S[qb][i]);
    else if (kind == 1) HS_MUL(P[qb][i], S[qb][i]);
    else HS_CVT(dsp[qb][i >> 2][i & 3], P[qb][2 * i], P[qb][2 * i + 1]);
  };
  // k = 0..3: (d block k & 1, k-step k >> 1)
  auto dq_mfma = [&](int k, int qb) __attribute__((always_inline)) {
    const int db = k & 1, s2 = k >> 1;
    HS_MFMA_G(dq[db][qb], cat44(ktr[0][db][s2][0], ktr[0][db][s2][1]), __builtin_bit_cast(bf16x8, dsp[qb][s2]));
  };
  auto mfma_gap = [&](int g) __attribute__((always_inline)) {
    if (g < 4) {
      if (g == 0) HS_MFMA_C0(S[0], kr[0], qf[0][0], NL[0]); else HS_MFMA_C(S[0], kr[g], qf[0][g]);
    } else if (g < 8) {
      if (g == 4) HS_MFMA_C0(P[0], vr[0], df[0][0], ND[0]); else HS_MFMA_C(P[0], vr[g - 4], df[0][g - 4]);
    } else if (g < 12) {
      dq_mfma(g - 8, 1);
    } else if (g < 16) {
      if (g == 12) HS_MFMA_C0(S[1], kr[0], qf[1][0], NL[1]); else HS_MFMA_C(S[1], kr[g - 12], qf[1][g - 12]);
    } else if (g < 20) {
      if (g == 16) HS_MFMA_C0(P[1], vr[0], df[1][0], ND[1]); else HS_MFMA_C(P[1], vr[g - 16], df[1][g - 16]);
    } else {
      dq_mfma(g - 20, 0);
    }
  };

  // One 32-key half (rows r0i of slot soff); the next half's rows are rows nr0i of slot nsoff. LDS reads: transposed
  // K at 12-19, the next half's K rows at 20-23; DQ_EARLY (round 6): the next half's V rows there too, 8 gaps before
  // the dP^T chain of block 0 instead of 4 (reloaded 1-4 gaps after their last read by block 1's chain: no extra
  // registers); else V rows at gaps 0-3.
  auto half = [&](int soff, int r0i, int nsoff, int nr0i, auto hook) __attribute__((always_inline)) {
#pragma unroll
    for (int g = 0; g < 24; ++g) {
      mfma_gap(g);
      // gaps 9 / 21 multiply the dP^T chain of block 0 / 1 (last MFMA at gap 7 / 19): 12 wait states by
      // instruction count
      if (g == 9 || g == 21) asm volatile("s_nop 5" ::: "memory");
#pragma unroll
      for (int o = 0; o < 4; ++o) valu_op(DQ_SCHED[g][o], -1);
      if (g >= 12 && g < 20) {
        const int f = (g - 12) >> 1, part = (g - 12) & 1;
        ktr[0][f & 1][f >> 1][part] = trh(soff, r0i, f, part);
      }
      if constexpr (DQ_EARLY) {
        if (g >= 20) {
          kr[g - 20] = row(nsoff, nr0i, g - 20);
          vr[g - 20] = row(nsoff + HS_TILE_B, nr0i, g - 20);
        }
      } else {
        if (g < 4) vr[g] = row(soff + HS_TILE_B, r0i, g);
        else if (g >= 20) kr[g - 20] = row(nsoff, nr0i, g - 20);
      }
      hook(g);
    }
  };

  // register staging (as the forward's): tile t+1's pieces (loaded into AGPRs during tile
  // t-1) are stored at gaps 1-7 of tile t's half 0, tile t+2's loaded at gaps 9-15; half 1's barrier publishes t+1
  u32x4 stg[4];
  const unsigned wst = ring.lds0 + 2048 * wave + 16 * lane;
  auto ld_piece = [&](int t, int i) __attribute__((always_inline)) {
    stg[i] = hs_ld16(ring.rsrc(i), ring.voff(i), ring.soff(t, i));
  };
  // prologue: tile 0 by LDS-DMA, tile 1 into the staging registers; wait, publish tile 0; K rows of half 0
  ring.dma(0, 0); ring.dma(0, 1); ring.dma(0, 2); ring.dma(0, 3);
  ld_piece(1, 0); ld_piece(1, 1); ld_piece(1, 2); ld_piece(1, 3);
  hs_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    kr[ks] = row(0, 0, ks);
    if (DQ_EARLY) vr[ks] = row(HS_TILE_B, 0, ks);
  }
  __builtin_amdgcn_s_waitcnt(LGKM0_WAIT);   // (see the dK/dV kernel's loop header)

  // SL >= 0: tile t sits in ring slot SL (compile-time: DS immediates); SL < 0: slot t & 3 at run time
  auto tile = [&](auto SL, int t) __attribute__((always_inline)) {
    constexpr int sl = decltype(SL)::value;
    const int soff = sl >= 0 ? sl * HS_SLOT_B : (t & (HS_NSLOT - 1)) * HS_SLOT_B;
    const int nsoff = sl >= 0 ? ((sl + 1) & (HS_NSLOT - 1)) * HS_SLOT_B : ((t + 1) & (HS_NSLOT - 1)) * HS_SLOT_B;
    // tile t+1 is published at gap 6 of half 1 (its first reader: the K rows at gaps 20-23)
    auto stage = [&](int g) __attribute__((always_inline)) {
      if (t + 1 < nkt4 && g == 6) __builtin_amdgcn_s_barrier();
    };
    auto stage0 = [&](int g) __attribute__((always_inline)) {
      if (g == 1) hs_vmcnt<0>();   // tile t+1's pieces (loaded a tile ago)
      if (g < 8 && (g & 1)) {
        constexpr int S1 = sl >= 0 ? ((sl + 1) & (HS_NSLOT - 1)) * HS_SLOT_B : 0;
        const unsigned base = sl >= 0 ? wst : wst + (unsigned)(((t + 1) & (HS_NSLOT - 1)) * HS_SLOT_B);
        switch (g) {
          case 1: hs_st16<S1>(base, stg[0]); break;
          case 3: hs_st16<S1 + 1024>(base, stg[1]); break;
          case 5: hs_st16<S1 + HS_TILE_B>(base, stg[2]); break;
          default: hs_st16<S1 + HS_TILE_B + 1024>(base, stg[3]); break;
        }
      } else if (g >= 9 && g < 16 && (g & 1)) {
        ld_piece(t + 2, (g - 9) >> 1);
      }
    };
    half(soff, 0, soff, 1, stage0);
    half(soff, 1, nsoff, 0, stage);
  };
  // the key tiles padded to a multiple of 4 (ring slots as DS immediates, no run-time-slot remainder loop, whose
  // second copy of the loop state spilled): tiles past L hold zero K / V rows (the staging loads' buffer range), so
  // their dS meets K^T = 0 and adds nothing to dQ^T
  for (int t = 0; t < nkt4; t += 4) {   // t & 3 == 0 here
    tile(std::integral_constant<int, 0>{}, t);
    tile(std::integral_constant<int, 1>{}, t + 1);
    tile(std::integral_constant<int, 2>{}, t + 2);
    tile(std::integral_constant<int, 3>{}, t + 3);
  }
  hs_vmcnt<0>();   // the last tiles' staging loads (past the end: zeros) retire
  // query block 1 of the last half: its remaining VALU (wrapped into gaps 0-5) and its dQ^T
#pragma unroll
  for (int g = 0; g < 12; ++g) {
#pragma unroll
    for (int o = 0; o < 4; ++o) valu_op(DQ_SCHED[g][o], 1);
    if (g >= 8) {
      asm volatile("s_nop 1" ::: "memory");
      dq_mfma(g - 8, 1);   // the last half is a half 1
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
  // the accumulators are read only after the last MFMAs completed: without this the compiler may move its
  // v_accvgpr_read above the s_nops (nothing else orders them)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) asm volatile("" : "+a"(dq[i][j]));

  const float sc = a.scale;
  // the lane's query re-derived here, not kept from the prologue: hoisted out of the loop, the epilogue's row
  // pointers were 8 VGPRs the full register file (DQ_EARLY) spills
  unsigned lane_e;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
  const int r32e = (int)lane_e & 31;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = qw0 + 32 * qb + r32e;
    if (q < L) {
      bf16* dqp = a.out + b * a.bs_out + (long long)q * a.rs_out + hh * a.hs;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = to_bf16(dq[db][qb][4 * g + j] * sc);
          *(bf16x4*)(dqp + 32 * db + 8 * g + 4 * h) = w;
        }
    }
  }
}

__global__ __launch_bounds__(HS_NW * 64, 1) void attn_bwd_dq_hs_kernel(AttnArgs a) { attn_bwd_dq_hs_body(a); }

// ---------------------------------------------------- backward: dQ kernel with 128 queries per wave (the wide dQ)
// attn_bwd_dq_hs_kernel's stream with four query blocks of 32 per wave (512 queries per workgroup): the 16 fragment
// reads of a 32-key half (4 K rows, 4 V rows, 8 transposed K halves), the tile's barrier, staging wait, four loads
// and four LDS stores feed 48 MFMAs instead of 24. Per half 48 gaps: block b's S~^T / dP^T chains at 12b .. 12b+7,
// the dQ^T MFMAs of block b-1 at 12b+8 .. 12b+11 (block 0's gaps: block 3 of the previous half); the S / dP / pack
// registers alternate between two sets (block b uses set b & 1, free again when block b+2's chains start); the VALU
// of each gap from DQ4_SCHED (tools/gen_dq_sched.py --nqb 4). LDS reads: transposed K at gaps 12-19 (before block 0's
// dQ^T at 20, after block 3's of the previous half at 8-11), the next half's K rows at 40-43 and V rows at 44-47
// (each 4 gaps after the last chain's read of the fragment).
// Registers: dQ^T 128 + Q~ 64 + dO 64 fill the AGPR half, so the staging registers are arch VGPRs, and the four
// -lse2 splats the narrow layout would need (64 registers) are one: with the query on the MFMA lane a per-query
// factor leaves the key sum,
//   dQ^T[d][q] = 2^(u - lse2_q) sum_k K^T[d][k] bf16(exp2(S~[k][q] - u) (dP[k][q] - delta_q))   for any per-lane u;
// u = the largest lse2 among the lane's (up to) four queries, so every exp2 is <= 1, all four S~ chains start from
// the one splat -u, and 2^(u - lse2_q) joins `scale` in the epilogue. -delta_q stays a per-block initial accumulator.
// A lane's spread u - lse2_q is bounded by SAFE_EXP2 = 64 (the forward's fixed-reference criterion: 2^63 of room
// before an f32 or bf16 under- or overflows): a workgroup with a lane past it writes 1 to its entry of the flag
// array behind the row constants (dq4_flags; every other workgroup writes 0) and returns, and
// attn_bwd_dq_hsfb_kernel, launched after it, runs the narrow stream for the flagged workgroups' queries.
constexpr int DQ4_NQB = 4;
constexpr int DQ4_NG = 12 * DQ4_NQB;          // gaps per half
constexpr int DQ4_QWG = HS_NW * 32 * DQ4_NQB;   // queries per workgroup
// gap  0: E3.8 E3.9
// gap  1: M3.8 M3.9 E3.10 C3.4
// gap  2: M3.10 E3.11 E3.12
// gap  3: M3.11 M3.12 C3.5 E3.13
// gap  4: E3.14 M3.13 E3.15 C3.6
// gap  5: M3.14 M3.15 E0.0 C3.7
// gap  6: E0.1 E0.2
// gap  7: E0.3 E0.4
// gap  8: E0.5 E0.6
// gap  9: M0.0 M0.1 M0.2 M0.3
// gap 10: C0.0 C0.1 M0.4 M0.5
// gap 11: M0.6 C0.2 E0.7 E0.8
// gap 12: M0.7 M0.8 C0.3 E0.9
// gap 13: E0.10 M0.9 E0.11 C0.4
// gap 14: M0.10 M0.11 E0.12 C0.5
// gap 15: M0.12 E0.13 E0.14
// gap 16: M0.13 M0.14 C0.6 E0.15
// gap 17: E1.0 M0.15 E1.1 C0.7
// gap 18: E1.2 E1.3
// gap 19: E1.4 E1.5
// gap 20: E1.6 E1.7
// gap 21: M1.0 M1.1 M1.2 M1.3
// gap 22: C1.0 C1.1 M1.4 M1.5
// gap 23: M1.6 M1.7 C1.2 C1.3
// gap 24: E1.8 E1.9
// gap 25: M1.8 M1.9 E1.10 C1.4
// gap 26: M1.10 E1.11 E1.12
// gap 27: M1.11 M1.12 C1.5 E1.13
// gap 28: E1.14 M1.13 E1.15 C1.6
// gap 29: E2.0 E2.1 M1.14 M1.15
// gap 30: E2.2 E2.3 C1.7
// gap 31: E2.4 E2.5
// gap 32: E2.6 E2.7
// gap 33: M2.0 M2.1 M2.2 M2.3
// gap 34: C2.0 C2.1 M2.4 M2.5
// gap 35: M2.6 M2.7 C2.2 C2.3
// gap 36: E2.8 E2.9
// gap 37: M2.8 M2.9 E2.10 C2.4
// gap 38: M2.10 E2.11 E2.12
// gap 39: M2.11 M2.12 C2.5 E2.13
// gap 40: E2.14 M2.13 E2.15 C2.6
// gap 41: E3.0 E3.1 M2.14 M2.15
// gap 42: E3.2 E3.3 C2.7
// gap 43: E3.4 E3.5
// gap 44: E3.6 E3.7
// gap 45: M3.0 M3.1 M3.2 M3.3
// gap 46: C3.0 C3.1 M3.4 M3.5
// gap 47: M3.6 M3.7 C3.2 C3.3
constexpr unsigned char DQ4_SCHED[48][4] = {
    {0x38, 0x39, 0xff, 0xff},
    {0x78, 0x79, 0x3a, 0xb4},
    {0x7a, 0x3b, 0x3c, 0xff},
    {0x7b, 0x7c, 0xb5, 0x3d},
    {0x3e, 0x7d, 0x3f, 0xb6},
    {0x7e, 0x7f, 0x00, 0xb7},
    {0x01, 0x02, 0xff, 0xff},
    {0x03, 0x04, 0xff, 0xff},
    {0x05, 0x06, 0xff, 0xff},
    {0x40, 0x41, 0x42, 0x43},
    {0x80, 0x81, 0x44, 0x45},
    {0x46, 0x82, 0x07, 0x08},
    {0x47, 0x48, 0x83, 0x09},
    {0x0a, 0x49, 0x0b, 0x84},
    {0x4a, 0x4b, 0x0c, 0x85},
    {0x4c, 0x0d, 0x0e, 0xff},
    {0x4d, 0x4e, 0x86, 0x0f},
    {0x10, 0x4f, 0x11, 0x87},
    {0x12, 0x13, 0xff, 0xff},
    {0x14, 0x15, 0xff, 0xff},
    {0x16, 0x17, 0xff, 0xff},
    {0x50, 0x51, 0x52, 0x53},
    {0x90, 0x91, 0x54, 0x55},
    {0x56, 0x57, 0x92, 0x93},
    {0x18, 0x19, 0xff, 0xff},
    {0x58, 0x59, 0x1a, 0x94},
    {0x5a, 0x1b, 0x1c, 0xff},
    {0x5b, 0x5c, 0x95, 0x1d},
    {0x1e, 0x5d, 0x1f, 0x96},
    {0x20, 0x21, 0x5e, 0x5f},
    {0x22, 0x23, 0x97, 0xff},
    {0x24, 0x25, 0xff, 0xff},
    {0x26, 0x27, 0xff, 0xff},
    {0x60, 0x61, 0x62, 0x63},
    {0xa0, 0xa1, 0x64, 0x65},
    {0x66, 0x67, 0xa2, 0xa3},
    {0x28, 0x29, 0xff, 0xff},
    {0x68, 0x69, 0x2a, 0xa4},
    {0x6a, 0x2b, 0x2c, 0xff},
    {0x6b, 0x6c, 0xa5, 0x2d},
    {0x2e, 0x6d, 0x2f, 0xa6},
    {0x30, 0x31, 0x6e, 0x6f},
    {0x32, 0x33, 0xa7, 0xff},
    {0x34, 0x35, 0xff, 0xff},
    {0x36, 0x37, 0xff, 0xff},
    {0x70, 0x71, 0x72, 0x73},
    {0xb0, 0xb1, 0x74, 0x75},
    {0x76, 0x77, 0xb2, 0xb3}};
static_assert(sizeof(DQ4_SCHED) == DQ4_NG * 4, "one row per gap");
__host__ __device__ constexpr unsigned char dq4_sched(int g, int o) { return DQ4_SCHED[g][o]; }

// per-workgroup flags of the wide dQ kernel, behind the (B, H, 2, L) row constants of the backward workspace:
// int32 [B][H][ceil(L / DQ4_QWG)], 1 = the workgroup left its queries to attn_bwd_dq_hsfb_kernel
__host__ __device__ inline long long dq4_flag_offset(int B, int H, int L) { return (long long)B * H * 2 * L; }   // floats
__device__ __forceinline__ int* dq4_flag(const AttnArgs& a, int wg, int hh, int b, int B) {
  const int nwg = (a.L + DQ4_QWG - 1) / DQ4_QWG;
  return (int*)(a.delta + dq4_flag_offset(B, a.H, a.L)) + ((long long)b * a.H + hh) * nwg + wg;
}

// the narrow stream for the queries of flagged wide workgroups (same grid as attn_bwd_dq_hs_kernel; two of its
// workgroups per wide one): their dQ is bitwise attn_bwd_dq_hs_kernel's
__global__ __launch_bounds__(HS_NW * 64, 1) void attn_bwd_dq_hsfb_kernel(AttnArgs a) {
  if (*dq4_flag(a, blockIdx.x / (DQ4_QWG / (HS_NW * 64)), blockIdx.y, blockIdx.z, gridDim.z) == 0) return;
  attn_bwd_dq_hs_body(a);
}

__global__ __launch_bounds__(HS_NW * 64, 1) void attn_bwd_dq_hs4_kernel(AttnArgs a) {
  constexpr int NQB = DQ4_NQB;
  constexpr int NG = DQ4_NG;
  constexpr int HALF_B = 32 * DH * 2;               // rows 32-63 of a tile: sw128 is invariant under 16-row steps
  __shared__ __attribute__((aligned(16))) char smem[HS_NSLOT * HS_SLOT_B];
  __shared__ int flagged_wg;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = blockIdx.y, b = blockIdx.z;
  const int L = a.L;
  const int h = lane >> 5, r32 = lane & 31;
  const int qw0 = blockIdx.x * DQ4_QWG + wave * (32 * NQB);
  const int nkt = (L + KT - 1) / KT;
  const int nkt4 = (nkt + 3) & ~3;
  if (tid == 0) flagged_wg = 0;

  // the row constants of the lane's four queries: -u = the smallest -lse2 among those below L, and the spread guard
  f32x16 NU, ND[NQB];
  {
    const float* ws = a.delta + ((long long)b * a.H + hh) * 2 * L;
    float lo = -NEG_BIG, hi = NEG_BIG;
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      const int q = qw0 + 32 * qb + r32;
      float nd = 0.f;
      if (q < L) {
        const float nl = ws[q];
        nd = ws[L + q];
        lo = fminf(lo, nl);
        hi = fmaxf(hi, nl);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) ND[qb][i] = nd;
    }
    const bool ok = hi - lo <= SAFE_EXP2;   // (a lane with no query: -2e30)
    const float nu = hi >= lo ? lo : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) NU[i] = nu;
    __syncthreads();
    if (!__all(ok) && lane == 0) flagged_wg = 1;
    __syncthreads();
    const int flagged = __builtin_amdgcn_readfirstlane(flagged_wg);
    if (tid == 0) *dq4_flag(a, blockIdx.x, hh, b, gridDim.z) = flagged;
    if (flagged) return;
  }
  HS_OPAQUE(NU);
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) HS_OPAQUE(ND[qb]);

  // Q~ / dO as B operands: lane holds X[qw0 + 32qb + r32][16ks + 8h + j] (Q prescaled into the exp2 domain)
  bf16x8 qf[NQB][4], df[NQB][4];
  {
    const bf16* qp = a.q + b * a.bs_q + hh * a.hs;
    const bf16* dop = a.dout + b * a.bs_do + hh * a.hs;
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      const int q = qw0 + 32 * qb + r32;
      hs_load_b2(qf[qb], df[qb], qp, a.rs_q, dop, a.rs_do, q, L, h, a.c);
      hs_vmcnt<0>();   // (no compiler vmcnt wait inside the loop; per block: the fragments go to AGPRs at once)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) { HS_TO_AGPR(qf[qb][ks]); HS_TO_AGPR(df[qb][ks]); }
    }
  }

  // ---- K / V tile pieces (wave w: rows 16w .. 16w+15 of each, 1-KB pieces of 8 rows): tile 0 by LDS-DMA
  const int rs2k = a.rs_k * 2, rs2v = a.rs_v * 2;
  const HsRing ring = hs_ring(hs_rows_rsrc(a.k + b * a.bs_k + hh * a.hs, rs2k, L), rs2k,
                              hs_rows_rsrc(a.v + b * a.bs_v + hh * a.hs, rs2v, L), rs2v, lane, wave, smem);

  // LDS byte offsets of the fragment reads of rows 0-31 within a ring slot (opaque lane registers, as the narrow
  // kernel's); rows 32-63 and the ring slot are DS immediates
  unsigned row_off[4], tr_off[4][2];   // [k-step | fragment][part]
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    row_off[k] = 2 * sw128(r32, 16 * k + 8 * h);
    HS_OPAQUE(row_off[k]);
#pragma unroll
    for (int part = 0; part < 2; ++part) {   // fragment k = (d block k & 1, k-step k >> 1)
      const int rw = 16 * (k >> 1) + 4 * h + ((lane & 15) >> 2) + 8 * part;
      const int col = 32 * (k & 1) + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
      tr_off[k][part] = 2 * sw128(rw, col);
      HS_OPAQUE(tr_off[k][part]);
    }
  }
  auto row = [&](int soff, int r0i, int ks) __attribute__((always_inline)) {   // soff: slot (+ HS_TILE_B for V) bytes
    return *(const bf16x8*)(smem + row_off[ks] + (soff + r0i * HALF_B));
  };
  auto trh = [&](int soff, int r0i, int f, int part) __attribute__((always_inline)) {
    return lds_tr4((const bf16*)(smem + tr_off[f][part] + (soff + r0i * HALF_B)));
  };

  f32x16 dq[2][NQB];           // [d block][query block]: dQ^T, lane = query, rows d = 32db + (i&3) + 8(i>>2) + 4h
  f32x16 S[2], P[2];           // [set]: S~^T - u, dP^T - delta (rows = the half's 32 keys)
  u32x4 dsp[2][2];             // [set][k-step] bf16 dS^T packs
  bf16x4 ktr[2][2][2];         // [d block][k-step][half of the fragment] transposed K (keys as the k index)
  // zeros: the first half's gaps 0-11 run block 3 of a half that does not exist (set 1: dS = exp2(0) * 0)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    S[i] = P[i] = f32x16{};
    HS_OPAQUE(S[i]);
    HS_OPAQUE(P[i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      dsp[i][j] = u32x4{};
      HS_OPAQUE(dsp[i][j]);
#pragma unroll
      for (int k = 0; k < 2; ++k) { ktr[i][j][k] = bf16x4{}; HS_OPAQUE(ktr[i][j][k]); }
    }
#pragma unroll
    for (int j = 0; j < NQB; ++j) { dq[i][j] = f32x16{}; HS_TO_AGPR(dq[i][j]); }
  }
  bf16x8 kr[4], vr[4];         // K / V row fragments (A operands of the chains)

  auto valu_op = [&](unsigned char c, int only_qb) __attribute__((always_inline)) {
    if (c == 0xFF) return;
    const int kind = c >> 6, qb = (c >> 4) & 3, st = qb & 1, i = c & 15;
    if (only_qb >= 0 && qb != only_qb) return;
    if (kind == 0) HS_EXP(S[st][i]);
    else if (kind == 1) HS_MUL(P[st][i], S[st][i]);
    else HS_CVT(dsp[st][i >> 2][i & 3], P[st][2 * i], P[st][2 * i + 1]);
  };
  // k = 0..3: (d block k & 1, k-step k >> 1)
  auto dq_mfma = [&](int k, int qb) __attribute__((always_inline)) {
    const int db = k & 1, s2 = k >> 1;
    HS_MFMA_G(dq[db][qb], cat44(ktr[db][s2][0], ktr[db][s2][1]), __builtin_bit_cast(bf16x8, dsp[qb & 1][s2]));
  };
  auto mfma_gap = [&](int g) __attribute__((always_inline)) {
    const int bq = g / 12, r = g % 12, st = bq & 1;
    if (r < 4) {
      if (r == 0) HS_MFMA_C0(S[st], kr[0], qf[bq][0], NU); else HS_MFMA_C(S[st], kr[r], qf[bq][r]);
    } else if (r < 8) {
      if (r == 4) HS_MFMA_C0(P[st], vr[0], df[bq][0], ND[bq]); else HS_MFMA_C(P[st], vr[r - 4], df[bq][r - 4]);
    } else {
      dq_mfma(r - 8, (bq + NQB - 1) % NQB);
    }
  };

  // One 32-key half (rows r0i of slot soff); the next half's rows are rows nr0i of slot nsoff
  constexpr int KR0 = NG - 8, VR0 = NG - 4;
  auto half = [&](int soff, int r0i, int nsoff, int nr0i, auto hook) __attribute__((always_inline)) {
    hs_for_gaps([&](auto G) __attribute__((always_inline)) {
      constexpr int g = decltype(G)::value;
      mfma_gap(g);
      // gap 12b+9 multiplies the dP^T chain of block b (last MFMA at 12b+7): 12 wait states by instruction count
      if (g % 12 == 9) asm volatile("s_nop 5" ::: "memory");
      valu_op(dq4_sched(g, 0), -1);
      valu_op(dq4_sched(g, 1), -1);
      valu_op(dq4_sched(g, 2), -1);
      valu_op(dq4_sched(g, 3), -1);
      if constexpr (g >= 12 && g < 20) {
        constexpr int f = (g - 12) >> 1, part = (g - 12) & 1;
        ktr[f & 1][f >> 1][part] = trh(soff, r0i, f, part);
      } else if constexpr (g >= KR0 && g < KR0 + 4) {
        kr[g - KR0] = row(nsoff, nr0i, g - KR0);
      } else if constexpr (g >= VR0) {
        vr[g - VR0] = row(nsoff + HS_TILE_B, nr0i, g - VR0);
      }
      hook(g);
    }, std::make_integer_sequence<int, NG>{});
  };

  // register staging as the narrow kernel's, in arch VGPRs: tile t+1's pieces (loaded during tile t-1) are stored at
  // gaps 1-7 of tile t's half 0, tile t+2's loaded at gaps 9-15; half 1's barrier publishes t+1
  u32x4 stg[4];
  const unsigned wst = ring.lds0 + 2048 * wave + 16 * lane;
  auto ld_piece = [&](int t, int i) __attribute__((always_inline)) {
    stg[i] = hs_ld16v(ring.rsrc(i), ring.voff(i), ring.soff(t, i));
  };
  // prologue: tile 0 by LDS-DMA, tile 1 into the staging registers; wait, publish tile 0; K / V rows of half 0
  ring.dma(0, 0); ring.dma(0, 1); ring.dma(0, 2); ring.dma(0, 3);
  ld_piece(1, 0); ld_piece(1, 1); ld_piece(1, 2); ld_piece(1, 3);
  hs_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    kr[ks] = row(0, 0, ks);
    vr[ks] = row(HS_TILE_B, 0, ks);
  }
  __builtin_amdgcn_s_waitcnt(LGKM0_WAIT);

  auto tile = [&](auto SL, int t) __attribute__((always_inline)) {   // tile t sits in ring slot SL (DS immediates)
    constexpr int sl = decltype(SL)::value;
    constexpr int soff = sl * HS_SLOT_B, nsoff = ((sl + 1) & (HS_NSLOT - 1)) * HS_SLOT_B;
    // tile t+1 is published at gap 6 of half 1 (its first reader: the K rows at gaps 40-43)
    auto stage = [&](int g) __attribute__((always_inline)) {
      if (t + 1 < nkt4 && g == 6) __builtin_amdgcn_s_barrier();
    };
    auto stage0 = [&](int g) __attribute__((always_inline)) {
      if (g == 1) hs_vmcnt<0>();   // tile t+1's pieces (loaded a tile ago)
      if (g < 8 && (g & 1)) {
        switch (g) {
          case 1: hs_st16v<nsoff>(wst, stg[0]); break;
          case 3: hs_st16v<nsoff + 1024>(wst, stg[1]); break;
          case 5: hs_st16v<nsoff + HS_TILE_B>(wst, stg[2]); break;
          default: hs_st16v<nsoff + HS_TILE_B + 1024>(wst, stg[3]); break;
        }
      } else if (g >= 9 && g < 16 && (g & 1)) {
        ld_piece(t + 2, (g - 9) >> 1);
      }
    };
    half(soff, 0, soff, 1, stage0);
    half(soff, 1, nsoff, 0, stage);
  };
  // key tiles padded to a multiple of 4, as the narrow kernel: zero K rows past L add nothing to dQ^T
  for (int t = 0; t < nkt4; t += 4) {   // t & 3 == 0 here
    tile(std::integral_constant<int, 0>{}, t);
    tile(std::integral_constant<int, 1>{}, t + 1);
    tile(std::integral_constant<int, 2>{}, t + 2);
    tile(std::integral_constant<int, 3>{}, t + 3);
  }
  hs_vmcnt<0>();   // the last tiles' staging loads (past the end: zeros) retire
  // query block 3 of the last half: its remaining VALU (wrapped into gaps 0-5) and its dQ^T
#pragma unroll
  for (int g = 0; g < 12; ++g) {
#pragma unroll
    for (int o = 0; o < 4; ++o) valu_op(dq4_sched(g, o), NQB - 1);
    if (g >= 8) {
      asm volatile("s_nop 1" ::: "memory");
      dq_mfma(g - 8, NQB - 1);
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {   // read only after the last MFMAs completed
    asm volatile("" : "+a"(dq[0][qb]));
    asm volatile("" : "+a"(dq[1][qb]));
  }

  // dQ = scale 2^(u - lse2_q) dQ^T. The lane's queries and row constants are re-derived here, not kept across the loop
  unsigned lane_e;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
  const int r32e = (int)lane_e & 31, he = (int)lane_e >> 5;
  const float* wse = a.delta + ((long long)b * a.H + hh) * 2 * L;
  float nle[NQB], lo = -NEG_BIG;
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int q = qw0 + 32 * qb + r32e;
    nle[qb] = q < L ? wse[q] : -NEG_BIG;
    lo = fminf(lo, nle[qb]);
  }
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int q = qw0 + 32 * qb + r32e;
    if (q < L) {
      const float sc = a.scale * exp2_fast(nle[qb] - lo);   // u - lse2_q = (-lse2_q) - (-u), in [0, 64]
      bf16* dqp = a.out + b * a.bs_out + (long long)q * a.rs_out + hh * a.hs;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = to_bf16(dq[db][qb][4 * g + j] * sc);
          *(bf16x4*)(dqp + 32 * db + 8 * g + 4 * he) = w;
        }
    }
  }
}

// ------------------------------------------------ forward: one wave per SIMD, placed MFMA / VALU / LDS stream
// The placed-stream structure of the backward kernels for O = softmax(Q K^T) V (backbone_vit.py:191-201): a workgroup =
// 4 waves x 64 queries (two query blocks of 32 on the MFMA lane), Q~ = c q fragments and the O^T accumulators in
// AGPRs, K | V tiles of 64 keys in a 4-slot LDS ring (tile t+1 stored from staging registers during tile t).
// Max-free softmax with one reference per query: m = the exact row max over the first key tile, which every chain
// starts from (-m as the initial accumulator), valid while ||q~|| max||k|| - m <= 64 over the whole key range (then
// p <= 2^64, exact in f32 sums and bf16 P: the attn_fwd2_kernel criterion, checked once per workgroup from the
// per-tile key norms); a workgroup outside it takes the exact online-softmax loop below (rescaled per 32 keys).

// Row sums on the matrix pipe (round 6): the 32 v_add_f32 per half of the round-4 stream (a quarter of its VALU issue)
// are replaced by 4 v_mfma_f32_16x16x32_bf16 that sum the bf16 P^T packs the PV MFMAs read anyway: with the pack as
// the B operand (lane l = 16 g + n holds 8 keys of query 16 (g & 1) + n) and A = a 0/1 selector (row 0 sums the lane
// groups g = 0, 2: query n; row 1 the groups 1, 3: query 16 + n), D rows 0 / 1 accumulate l of the block's 32 queries.
// The denominator is then the sum of the same bf16-rounded P the numerator uses. The MFMA's accumulation is not an
// f32 RNE sum (a running 65536-key row sum on it came out up to 1.3 % low against an exact sum: bits of the new
// products below the accumulator's ulp are dropped, a bias in one direction when every term is positive), so each
// half's two row-sum MFMAs start from a zero accumulator and their result is added into an f32 running sum by a
// v_add_f32 per block and row half (A ops: 4 per half instead of 32). Per half (20 gaps):
//   0-3 S^T chain of block 0 | 4, 5, 7, 8 O^T += V^T P^T of block 1 (previous half), 6 / 9 its row sums (k-step 0 / 1)
//   10-13 S^T chain of block 1 | 14, 15, 17, 18 O^T of block 0, 16 / 19 its row sums,
// against 32 exp2 and 16 packs placed by FW_SCHED_R (tools/gen_fwd_sched.py --rsum: <= 2 exp2 + 1 pack beside a
// 32x32x16 MFMA, one op beside a 16x16x32; E starts two gaps after its chain, packs before the MFMAs that read them).
constexpr int FW_NG = 20;          // gaps per half
constexpr int FW_START_E1 = 15;    // first gap of block 1's exps
// gap  0 S0: E1.6 E1.7
// gap  1 S0: E1.8 E1.9 C1.3
// gap  2 S0: E1.10 E1.11 C1.4 A0.0
// gap  3 S0: E1.12 E1.13 C1.5 A0.1
// gap  4 P1: E1.14 E1.15 C1.6
// gap  5 P1: C1.7 E0.0 E0.1
// gap  6 R1: C0.0
// gap  7 P1: E0.2 E0.3
// gap  8 P1: E0.4 E0.5 C0.1
// gap  9 R1: C0.2
// gap 10 S1: E0.6 E0.7
// gap 11 S1: E0.8 E0.9 C0.3
// gap 12 S1: E0.10 E0.11 C0.4 A1.0
// gap 13 S1: E0.12 E0.13 C0.5 A1.1
// gap 14 P0: E0.14 E0.15 C0.6
// gap 15 P0: C0.7 E1.0 E1.1
// gap 16 R0: C1.0
// gap 17 P0: E1.2 E1.3
// gap 18 P0: E1.4 E1.5 C1.1
// gap 19 R0: C1.2
constexpr unsigned char FW_SCHED_R[20][4] = {
    {0x26, 0x27, 0xff, 0xff},
    {0x28, 0x29, 0xa3, 0xff},
    {0x2a, 0x2b, 0xa4, 0x40},
    {0x2c, 0x2d, 0xa5, 0x41},
    {0x2e, 0x2f, 0xa6, 0xff},
    {0xa7, 0x00, 0x01, 0xff},
    {0x80, 0xff, 0xff, 0xff},
    {0x02, 0x03, 0xff, 0xff},
    {0x04, 0x05, 0x81, 0xff},
    {0x82, 0xff, 0xff, 0xff},
    {0x06, 0x07, 0xff, 0xff},
    {0x08, 0x09, 0x83, 0xff},
    {0x0a, 0x0b, 0x84, 0x60},
    {0x0c, 0x0d, 0x85, 0x61},
    {0x0e, 0x0f, 0x86, 0xff},
    {0x87, 0x20, 0x21, 0xff},
    {0xa0, 0xff, 0xff, 0xff},
    {0x22, 0x23, 0xff, 0xff},
    {0x24, 0x25, 0xa1, 0xff},
    {0xa2, 0xff, 0xff, 0xff}};
constexpr int FW_CAP = 4;
__host__ __device__ constexpr unsigned char fw_sched(int g, int o) { return FW_SCHED_R[g][o]; }

// initial S^T of query block 1 before the first half: the exps of block 1 that the schedule wraps into the next half
// (E1.i in gaps before FW_START_E1) see NEG_BIG (exp2 -> 0); the elements exponentiated in the previous half's last
// gaps are already "exponentiated": 0. Either way the first half sums and packs zeros for the missing half -1.
__host__ __device__ constexpr bool fw_wrapped_exp(int i) {
  for (int g = 0; g < FW_START_E1; ++g)
    for (int o = 0; o < FW_CAP; ++o)
      if (fw_sched(g, o) == (0x20 | i)) return true;
  return false;
}

// Timing probes (variant builds only; results are wrong): LCI_FWD_PROBE bit 0 drops the per-tile barrier, bit 1 the
// wait for tile t+1's staging loads -- what the two synchronisation points of the stream cost
#ifndef LCI_FWD_PROBE
#define LCI_FWD_PROBE 0
#endif
__global__ __launch_bounds__(HS_NW * 64, 1) void attn_fwd_hs_kernel(AttnArgs a, const float* knorm) {
  __shared__ __attribute__((aligned(16))) char smem[HS_NSLOT * HS_SLOT_B];
  __shared__ int unsafe_wg;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = blockIdx.y, b = blockIdx.z;
  const int L = a.L;
  const int h = lane >> 5, r32 = lane & 31;
  const int qw0 = blockIdx.x * (HS_NW * 64) + wave * 64;
  const int nkt = (L + KT - 1) / KT;
  if (tid == 0) unsafe_wg = 0;

  // Q~ = c q as B operands: lane holds q~[qw0 + 32 qb + r32][16 ks + 8h + j]; qn = ||q~|| of the lane's query
  bf16x8 qf[2][4];
  float qn[2];
  {
    const bf16* qp = a.q + b * a.bs_q + hh * a.hs;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int q = qw0 + 32 * qb + r32;
      float ss = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 t{};
        if (q < L) t = *(const bf16x8*)(qp + (long long)q * a.rs_q + 16 * ks + 8 * h);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          t[j] = to_bf16(to_f32(t[j]) * a.c);
          ss += to_f32(t[j]) * to_f32(t[j]);
        }
        qf[qb][ks] = t;
      }
      qn[qb] = sqrtf(wave_sum_xor32(ss));
    }
  }
  // the key-norm bound over the whole key range, and the exact row max of the first key tile
  const float* kn = knorm + ((long long)b * a.H + hh) * nkt;
  float kmax = 0.f;
  for (int t = lane; t < nkt; t += 64) kmax = fmaxf(kmax, kn[t]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) kmax = fmaxf(kmax, __shfl_xor(kmax, o));
  const bf16* kp = a.k + b * a.bs_k + hh * a.hs;
  const bf16* vp = a.v + b * a.bs_v + hh * a.hs;
  float m[2];
  {
    bf16x8 k0[2][4];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int key = 32 * kb + r32;
        k0[kb][ks] = key < L ? *(const bf16x8*)(kp + (long long)key * a.rs_k + 16 * ks + 8 * h) : bf16x8{};
      }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float mx = NEG_BIG;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 sc = {};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) sc = mfma32(k0[kb][ks], qf[qb][ks], sc);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (32 * kb + (i & 3) + 8 * (i >> 2) + 4 * h < L) mx = fmaxf(mx, sc[i]);
      }
      m[qb] = wave_max_xor32(mx);
    }
  }
  __syncthreads();
  if (!__all(qn[0] * kmax - m[0] <= SAFE_EXP2 && qn[1] * kmax - m[1] <= SAFE_EXP2) && lane == 0) unsafe_wg = 1;
  __syncthreads();
  const int unsafe = __builtin_amdgcn_readfirstlane(unsafe_wg);

  if (unsafe) {
    // exact online softmax, 32 keys at a time (operands straight from global memory: the rare path)
    f32x16 o[2][2];
    float mr[2] = {m[0], m[1]}, lr[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) o[i][j] = f32x16{};
    for (int k0 = 0; k0 < L; k0 += 32) {
      bf16x8 kr[4], vt[2][2];
      const int key = k0 + r32;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        kr[ks] = key < L ? *(const bf16x8*)(kp + (long long)key * a.rs_k + 16 * ks + 8 * h) : bf16x8{};
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) {   // V^T: lane (h, d) holds V[key k(8h + j)][d], k-order of the P packs
            const int kk = k0 + 16 * s2 + (j & 3) + 8 * (j >> 2) + 4 * h;
            vt[db][s2][j] = kk < L ? vp[(long long)kk * a.rs_v + 32 * db + r32] : to_bf16(0.f);
          }
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        f32x16 sc = {};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) sc = mfma32(kr[ks], qf[qb][ks], sc);
        float mx = NEG_BIG;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (k0 + (i & 3) + 8 * (i >> 2) + 4 * h >= L) sc[i] = NEG_BIG;
          mx = fmaxf(mx, sc[i]);
        }
        const float mn = fmaxf(mr[qb], wave_max_xor32(mx));
        const float alpha = exp2_fast(mr[qb] - mn);
        mr[qb] = mn;
        lr[qb] *= alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o[qb][0][i] *= alpha; o[qb][1][i] *= alpha; }
        bf16x8 pk[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = exp2_fast(sc[i] - mn);
          lr[qb] += p;
          pk[i >> 3][i & 7] = to_bf16(p);
        }
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) o[qb][db] = mfma32(vt[db][s2], pk[s2], o[qb][db]);
      }
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int q = qw0 + 32 * qb + r32;
      const float lt = wave_sum_xor32(lr[qb]);
      if (q < L) {
        const float inv = 1.f / lt;
        bf16* op = a.out + b * a.bs_out + (long long)q * a.rs_out + hh * a.hs;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            bf16x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = to_bf16(o[qb][db][4 * g + j] * inv);
            *(bf16x4*)(op + 32 * db + 8 * g + 4 * h) = w;
          }
        if (h == 0) a.lse2[((long long)b * a.H + hh) * L + q] = mr[qb] + __log2f(lt);
      }
    }
    return;
  }

  // ---- the placed stream
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) HS_TO_AGPR(qf[i][j]);
  const int rs2k = a.rs_k * 2, rs2v = a.rs_v * 2;
  const HsRing ring = hs_ring(hs_rows_rsrc(kp, rs2k, L), rs2k, hs_rows_rsrc(vp, rs2v, L), rs2v, lane, wave, smem);
  // LDS byte offsets of every distinct fragment read within a ring slot, computed once (the swizzle XOR per row
  // included) and kept opaque: with the slot a compile-time constant (the 4-tile unroll below) each read is then one
  // ds_read with a lane register and an immediate, no address VALU in the loop
  unsigned row_off[2][4], tr_off[2][4][2];   // [rows 0-31 | 32-63][k-step | fragment][part]
#pragma unroll
  for (int r0i = 0; r0i < 2; ++r0i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      row_off[r0i][k] = 2 * sw128(32 * r0i + r32, 16 * k + 8 * h);
      HS_OPAQUE(row_off[r0i][k]);
#pragma unroll
      for (int part = 0; part < 2; ++part) {   // fragment k = (d block k & 1, k-step k >> 1)
        const int rw = 32 * r0i + 16 * (k >> 1) + 4 * h + ((lane & 15) >> 2) + 8 * part;
        const int col = 32 * (k & 1) + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        tr_off[r0i][k][part] = HS_TILE_B + 2 * sw128(rw, col);
        HS_OPAQUE(tr_off[r0i][k][part]);
      }
    }
  auto row = [&](int soff, int r0i, int ks) __attribute__((always_inline)) {
    return *(const bf16x8*)(smem + row_off[r0i][ks] + soff);
  };
  auto trh = [&](int soff, int r0i, int f, int part) __attribute__((always_inline)) {
    return lds_tr4((const bf16*)(smem + tr_off[r0i][f][part] + soff));
  };

  f32x16 o[2][2];     // [query block][d block] O^T, lane = query, rows d = 32 db + (i & 3) + 8 (i >> 2) + 4h
  f32x16 S[2];        // [query block] S~^T - m, then P (rows = the half's 32 keys)
  f32x16 NM[2];       // -m splat: the chains' initial accumulator
  u32x4 pp[2][2];     // [query block][k-step] bf16 P^T packs
  bf16x4 vt[2][2][2][2];   // [set][d block][k-step][half of the fragment] transposed V (keys as the k index)
  bf16x8 kr[4];       // K row fragments (A operands of the chains)
  float lp[2][2];     // [query block][row half] running f32 row sums (lanes 0-15: queries 16 s + lane)
  f32x4 rs[2];        // [query block] the half's row-sum partial on the matrix pipe: D rows 0 / 1 in lanes 0-15
  bf16x8 sel;         // 16x16x32 A operand: row 0 selects lane groups 0 / 2, row 1 groups 1 / 3 (all 8 k per lane)
  {
    const int m16 = lane & 15, g16 = lane >> 4;
    const float one = (m16 == 0 && (g16 & 1) == 0) || (m16 == 1 && (g16 & 1) == 1) ? 1.f : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sel[j] = to_bf16(one);
    HS_TO_AGPR(sel);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      NM[i][e] = -m[i];
      S[i][e] = (i == 1 && fw_wrapped_exp(e)) ? NEG_BIG : 0.f;
    }
    HS_OPAQUE(NM[i]);
    HS_OPAQUE(S[i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      o[i][j] = f32x16{};
      HS_TO_AGPR(o[i][j]);
      pp[i][j] = u32x4{};
      HS_OPAQUE(pp[i][j]);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        vt[0][i][j][k] = vt[1][i][j][k] = bf16x4{};
        HS_OPAQUE(vt[0][i][j][k]);
        HS_OPAQUE(vt[1][i][j][k]);
      }
    }
    lp[i][0] = lp[i][1] = 0.f;
    rs[i] = f32x4{};
    HS_OPAQUE(rs[i]);
  }

  auto valu_op = [&](unsigned char cd, int only_qb) __attribute__((always_inline)) {
    if (cd == 0xFF) return;
    const int kind = cd >> 6, qb = (cd >> 5) & 1, i = cd & 31;
    if (only_qb >= 0 && qb != only_qb) return;
    if (kind == 0) HS_EXP(S[qb][i]);
    else if (kind == 1) {
      asm volatile("v_add_f32 %0, %0, %1" : "+v"(lp[qb][i]) : "v"(rs[qb][i]));
      // rows 2 / 3 of the accumulator are never read, but the next MFMA writes all four registers: keep them
      // allocated so that nothing else lives in them inside its hazard window
      if (i == 1) HS_KEEP(rs[qb]);
    } else HS_CVT(pp[qb][i >> 2][i & 3], S[qb][2 * i], S[qb][2 * i + 1]);
  };
  auto pv_mfma = [&](int k, int qb, int st) __attribute__((always_inline)) {   // k: (d block k & 1, k-step k >> 1)
    const int db = k & 1, s2 = k >> 1;
    HS_MFMA_G(o[qb][db], cat44(vt[st][db][s2][0], vt[st][db][s2][1]), __builtin_bit_cast(bf16x8, pp[qb][s2]));
  };
  // the half's row-sum partial of block qb: the column sums of its two P^T packs (k-step 0 starts from zero)
  auto rs_mfma = [&](int qb, int s2) __attribute__((always_inline)) {
    if (s2 == 0)
      asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(rs[qb]) : "a"(sel), "v"(pp[qb][0]));
    else
      asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(rs[qb]) : "a"(sel), "v"(pp[qb][1]));
  };
  auto mfma_gap = [&](int g, int C, const f32x16& i0, const f32x16& i1) __attribute__((always_inline)) {
    // 0-3 S0 | 4 5 (6) 7 8 (9) PV / row sums of block 1 | 10-13 S1 | 14 15 (16) 17 18 (19) PV / row sums of block 0
    if (g < 4) {
      if (g == 0) HS_MFMA_C0(S[0], kr[0], qf[0][0], i0); else HS_MFMA_C(S[0], kr[g], qf[0][g]);
    } else if (g < 10) {
      if (g == 6 || g == 9) rs_mfma(1, g == 9);
      else pv_mfma(g < 6 ? g - 4 : g - 5, 1, C ^ 1);
    } else if (g < 14) {
      if (g == 10) HS_MFMA_C0(S[1], kr[0], qf[1][0], i1); else HS_MFMA_C(S[1], kr[g - 10], qf[1][g - 10]);
    } else {
      if (g == 16 || g == 19) rs_mfma(0, g == 19);
      else pv_mfma(g < 16 ? g - 14 : g - 15, 0, C);
    }
  };

  // one 32-key half (rows 32 r0i of the slot at byte offset soff, V^T set SET): the transposed V fragments at gaps 0-7,
  // the next half's K rows (rows 32 nr0i of the slot at nsoff) at gaps 13-16, right behind the gap's MFMA
  auto half = [&](auto SET, auto FIXED, int soff, int r0i, int nsoff, int nr0i, const f32x16& i0, const f32x16& i1,
                  auto hook) __attribute__((always_inline)) {
    constexpr int C = decltype(SET)::value;
    constexpr bool FIXED_SLOT = decltype(FIXED)::value;
    constexpr int NG = FW_NG;
    constexpr int KR0 = 13;   // first gap of the next half's K-row reads (each fragment reloaded >= 3 gaps after the S1
                              // chain's last read of it)
    auto lds_reads = [&](int g) __attribute__((always_inline)) {
      if (g < 8) {
        const int f = g >> 1, part = g & 1;   // fragment f = (d block f & 1, k-step f >> 1)
        vt[C][f & 1][f >> 1][part] = trh(soff, r0i, f, part);
      } else if (g >= KR0 && g < KR0 + 4) {   // the next half's K rows
        kr[g - KR0] = row(nsoff, nr0i, g - KR0);
      }
    };
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      mfma_gap(g, C, i0, i1);
      if (g == 2) HS_KEEP(i0);    // the chain-start MFMAs read their initial accumulators as SrcC after issue
      if (g == 12) HS_KEEP(i1);
      // the gap's LDS read right behind its MFMA (one more wait state between a chain's last MFMA and the first exp
      // that reads it, and between an exp and a pack reading it across the gap boundary)
      lds_reads(g);
      // run-time-slot tiles (remainder, ragged last tile): the compiler may sink their LDS reads, so the wait states
      // between a chain's last MFMA and its first exp are padded explicitly
      if (!FIXED_SLOT && (g == 5 || g == 15)) asm volatile("s_nop 1" ::: "memory");
#pragma unroll
      for (int op = 0; op < FW_CAP; ++op) valu_op(fw_sched(g, op), -1);
      hook(g);
    }
  };

  // register staging: tile t+1's pieces (loaded into AGPRs during tile t-1) are stored to ring slot (t+1) & 3 at
  // gaps 1-7 of tile t's half 0 and tile t+2's loaded at gaps 9-15; the barrier of tile t's half 1 publishes tile
  // t+1. A piece costs a buffer load + a ds_write_b128 instead of an LDS-DMA issue (~56 cycles each, measured).
  // Pieces past the last tile read as zero (buffer range) into slots nobody reads.
  u32x4 stg[4];
  const unsigned wst = ring.lds0 + 2048 * wave + 16 * lane;
  auto ld_piece = [&](int t, int i) __attribute__((always_inline)) {
    stg[i] = hs_ld16(ring.rsrc(i), ring.voff(i), ring.soff(t, i));
  };
  // prologue: tile 0 by LDS-DMA, tile 1 into the staging AGPRs; wait for tile 0; K rows of its first half
  ring.dma(0, 0); ring.dma(0, 1); ring.dma(0, 2); ring.dma(0, 3);
  ld_piece(1, 0); ld_piece(1, 1); ld_piece(1, 2); ld_piece(1, 3);
  hs_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kr[ks] = row(0, 0, ks);
  __builtin_amdgcn_s_waitcnt(LGKM0_WAIT);

  // SL >= 0: tile t sits in ring slot SL (compile-time: immediates); SL < 0: slot t & 3 at run time
  auto tile = [&](auto SL, int t, const f32x16& a0, const f32x16& a1, const f32x16& b0, const f32x16& b1)
      __attribute__((always_inline)) {
    constexpr int sl = decltype(SL)::value;
    const int soff = sl >= 0 ? sl * HS_SLOT_B : (t & (HS_NSLOT - 1)) * HS_SLOT_B;
    const int nsoff = sl >= 0 ? ((sl + 1) & (HS_NSLOT - 1)) * HS_SLOT_B : ((t + 1) & (HS_NSLOT - 1)) * HS_SLOT_B;
    // tile t+1 is published at gap 6 of half 1 (first reader: the K rows at gaps 12-15)
    auto stage = [&](int g) __attribute__((always_inline)) {
      if (!(LCI_FWD_PROBE & 1) && t + 1 < nkt && g == 7) __builtin_amdgcn_s_barrier();
    };
    constexpr int LD0 = 11;   // tile t+2's loads at gaps 11, 13, 15, 17 (32x32x16 gaps)
    auto rstg = [&](int g) __attribute__((always_inline)) {
      if (!(LCI_FWD_PROBE & 2) && g == 1) hs_vmcnt<0>();   // tile t+1's pieces (loaded a tile ago)
      if (g < 8 && (g & 1)) {
        constexpr int S1 = sl >= 0 ? ((sl + 1) & (HS_NSLOT - 1)) * HS_SLOT_B : 0;
        const unsigned base = sl >= 0 ? wst : wst + (unsigned)(((t + 1) & (HS_NSLOT - 1)) * HS_SLOT_B);
        switch (g) {
          case 1: hs_st16<S1>(base, stg[0]); break;
          case 3: hs_st16<S1 + 1024>(base, stg[1]); break;
          case 5: hs_st16<S1 + HS_TILE_B>(base, stg[2]); break;
          default: hs_st16<S1 + HS_TILE_B + 1024>(base, stg[3]); break;
        }
      } else if (g >= LD0 && g < LD0 + 8 && ((g - LD0) & 1) == 0) {
        ld_piece(t + 2, (g - LD0) >> 1);
      }
    };
    half(std::integral_constant<int, 0>{}, std::bool_constant<(sl >= 0)>{}, soff, 0, soff, 1, a0, a1, rstg);
    half(std::integral_constant<int, 1>{}, std::bool_constant<(sl >= 0)>{}, soff, 1, nsoff, 0, b0, b1, stage);
  };
  const bool ragged = (L & (KT - 1)) != 0;
  const int nfast = ragged ? nkt - 1 : nkt;
  using IC0 = std::integral_constant<int, 0>;
  using IC1 = std::integral_constant<int, 1>;
  using IC2 = std::integral_constant<int, 2>;
  using IC3 = std::integral_constant<int, 3>;
  using ICR = std::integral_constant<int, -1>;
  int t = 0;
  for (; t + 4 <= nfast; t += 4) {   // t & 3 == 0 here
    tile(IC0{}, t, NM[0], NM[1], NM[0], NM[1]);
    tile(IC1{}, t + 1, NM[0], NM[1], NM[0], NM[1]);
    tile(IC2{}, t + 2, NM[0], NM[1], NM[0], NM[1]);
    tile(IC3{}, t + 3, NM[0], NM[1], NM[0], NM[1]);
  }
  for (; t < nfast; ++t) tile(ICR{}, t, NM[0], NM[1], NM[0], NM[1]);
  if (ragged) {   // the last tile: keys past L start from NEG_BIG (their K rows read as zero), so exp2 gives 0
    const int tl = nkt - 1;
    f32x16 M[2][2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          M[hf][qb][e] = tl * KT + 32 * hf + (e & 3) + 8 * (e >> 2) + 4 * h < L ? -m[qb] : NEG_BIG;
        HS_OPAQUE(M[hf][qb]);
      }
    asm volatile("s_nop 4" ::: "memory");
    tile(ICR{}, tl, M[0][0], M[0][1], M[1][0], M[1][1]);
  }
  hs_vmcnt<0>();   // the last tiles' staging loads (past the end: zeros) retire before the exit
  // query block 1 of the last half: its wrapped VALU and its PV (and row-sum) MFMAs
#pragma unroll
  for (int g = 0; g < 10; ++g) {
#pragma unroll
    for (int op = 0; op < FW_CAP; ++op) valu_op(fw_sched(g, op), 1);
    if (g >= 4) {
      asm volatile("s_nop 1" ::: "memory");
      if (g == 6 || g == 9) rs_mfma(1, g == 9);
      else pv_mfma(g < 6 ? g - 4 : g - 5, 1, 1);   // the last half is a half 1
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
  HS_OPAQUE(rs[0]);   // read only after the last MFMAs completed
  HS_OPAQUE(rs[1]);

#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = qw0 + 32 * qb + r32;
    // l of query 16 s + n sits in lane n, row s of the block's 16x16 accumulator (+ the last half's partials)
    const float s0 = lp[qb][0] + rs[qb][0], s1 = lp[qb][1] + rs[qb][1];
    const float l0 = __shfl(s0, r32 & 15), l1 = __shfl(s1, r32 & 15);
    const float lt = r32 < 16 ? l0 : l1;
    if (q < L) {
      const float inv = 1.f / lt;
      bf16* op = a.out + b * a.bs_out + (long long)q * a.rs_out + hh * a.hs;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = to_bf16(o[qb][db][4 * g + j] * inv);
          *(bf16x4*)(op + 32 * db + 8 * g + 4 * h) = w;
        }
      if (h == 0) a.lse2[((long long)b * a.H + hh) * L + q] = m[qb] + __log2f(lt);
    }
  }
}

// ------------------------------------------------ forward, wide: 128 queries per wave (four query blocks)
// attn_fwd_hs_kernel's stream with FW4_NQB = 4 query blocks of 32 per wave, 512 queries per workgroup: every K | V
// tile a workgroup stages (4 buffer loads + 4 ds_write_b128 per wave, one barrier, one staging wait) and every
// fragment a wave reads from LDS (4 K rows, 8 V^T halves per 32-key half) now feeds 32 large MFMAs instead of 16, so
// L2 -> LDS bytes, LDS instructions and synchronisation per MFMA are halved; the arithmetic per query is unchanged, in
// the same order (m, the chain's k-steps, the bf16 packs, the key order into O^T, the per-half row-sum MFMAs and f32
// adds), so O and lse2 are bitwise those of attn_fwd_hs_kernel wherever both take the same safe / unsafe path.
// Per half (40 gaps), block b = 0..3: gaps 10b .. 10b+3 the S^T chain of block b, 10b+4, +5, +7, +8 O^T += V^T P^T of
// block b-1 (block 3: of the previous half), 10b+6 / 10b+9 its row sums; the VALU of a block (FW4_SCHED_R,
// tools/gen_fwd_sched.py --nqb 4) is the two-block placement shifted by 10 gaps per block, so at most two blocks' S
// are live at a time. The row-sum adds of blocks 0 / 1 fall into the same half (gaps 22 / 23, 32 / 33), those of
// blocks 2 / 3 into the next (2 / 3, 12 / 13). The next half's K rows are read at gaps 33-36 (each fragment 3 gaps
// after the last chain's read of it). AGPRs: O^T 128, Q~ 64, selector 4, staging 16.
constexpr int FW4_NQB = 4;                 // query blocks of 32 per wave
constexpr int FW4_NG = 10 * FW4_NQB;       // gaps per half
constexpr int FW4_QWG = HS_NW * 32 * FW4_NQB;   // queries per workgroup
// gap  0 S0: E3.6 E3.7
// gap  1 S0: E3.8 E3.9 C3.3
// gap  2 S0: E3.10 E3.11 C3.4 A2.0
// gap  3 S0: E3.12 E3.13 C3.5 A2.1
// gap  4 P3: E3.14 E3.15 C3.6
// gap  5 P3: C3.7 E0.0 E0.1
// gap  6 R3: C0.0
// gap  7 P3: E0.2 E0.3
// gap  8 P3: E0.4 E0.5 C0.1
// gap  9 R3: C0.2
// gap 10 S1: E0.6 E0.7
// gap 11 S1: E0.8 E0.9 C0.3
// gap 12 S1: E0.10 E0.11 C0.4 A3.0
// gap 13 S1: E0.12 E0.13 C0.5 A3.1
// gap 14 P0: E0.14 E0.15 C0.6
// gap 15 P0: C0.7 E1.0 E1.1
// gap 16 R0: C1.0
// gap 17 P0: E1.2 E1.3
// gap 18 P0: E1.4 E1.5 C1.1
// gap 19 R0: C1.2
// gap 20 S2: E1.6 E1.7
// gap 21 S2: E1.8 E1.9 C1.3
// gap 22 S2: E1.10 E1.11 C1.4 A0.0
// gap 23 S2: E1.12 E1.13 C1.5 A0.1
// gap 24 P1: E1.14 E1.15 C1.6
// gap 25 P1: C1.7 E2.0 E2.1
// gap 26 R1: C2.0
// gap 27 P1: E2.2 E2.3
// gap 28 P1: E2.4 E2.5 C2.1
// gap 29 R1: C2.2
// gap 30 S3: E2.6 E2.7
// gap 31 S3: E2.8 E2.9 C2.3
// gap 32 S3: E2.10 E2.11 C2.4 A1.0
// gap 33 S3: E2.12 E2.13 C2.5 A1.1
// gap 34 P2: E2.14 E2.15 C2.6
// gap 35 P2: C2.7 E3.0 E3.1
// gap 36 R2: C3.0
// gap 37 P2: E3.2 E3.3
// gap 38 P2: E3.4 E3.5 C3.1
// gap 39 R2: C3.2
constexpr unsigned char FW4_SCHED_R[40][4] = {
    {0x36, 0x37, 0xff, 0xff},
    {0x38, 0x39, 0xb3, 0xff},
    {0x3a, 0x3b, 0xb4, 0x60},
    {0x3c, 0x3d, 0xb5, 0x61},
    {0x3e, 0x3f, 0xb6, 0xff},
    {0xb7, 0x00, 0x01, 0xff},
    {0x80, 0xff, 0xff, 0xff},
    {0x02, 0x03, 0xff, 0xff},
    {0x04, 0x05, 0x81, 0xff},
    {0x82, 0xff, 0xff, 0xff},
    {0x06, 0x07, 0xff, 0xff},
    {0x08, 0x09, 0x83, 0xff},
    {0x0a, 0x0b, 0x84, 0x70},
    {0x0c, 0x0d, 0x85, 0x71},
    {0x0e, 0x0f, 0x86, 0xff},
    {0x87, 0x10, 0x11, 0xff},
    {0x90, 0xff, 0xff, 0xff},
    {0x12, 0x13, 0xff, 0xff},
    {0x14, 0x15, 0x91, 0xff},
    {0x92, 0xff, 0xff, 0xff},
    {0x16, 0x17, 0xff, 0xff},
    {0x18, 0x19, 0x93, 0xff},
    {0x1a, 0x1b, 0x94, 0x40},
    {0x1c, 0x1d, 0x95, 0x41},
    {0x1e, 0x1f, 0x96, 0xff},
    {0x97, 0x20, 0x21, 0xff},
    {0xa0, 0xff, 0xff, 0xff},
    {0x22, 0x23, 0xff, 0xff},
    {0x24, 0x25, 0xa1, 0xff},
    {0xa2, 0xff, 0xff, 0xff},
    {0x26, 0x27, 0xff, 0xff},
    {0x28, 0x29, 0xa3, 0xff},
    {0x2a, 0x2b, 0xa4, 0x50},
    {0x2c, 0x2d, 0xa5, 0x51},
    {0x2e, 0x2f, 0xa6, 0xff},
    {0xa7, 0x30, 0x31, 0xff},
    {0xb0, 0xff, 0xff, 0xff},
    {0x32, 0x33, 0xff, 0xff},
    {0x34, 0x35, 0xb1, 0xff},
    {0xb2, 0xff, 0xff, 0xff}};
static_assert(sizeof(FW4_SCHED_R) == FW4_NG * 4, "one row per gap");
__host__ __device__ constexpr unsigned char fw4_sched(int g, int o) { return FW4_SCHED_R[g][o]; }
// initial S^T of the last query block (its VALU wraps into the next half), as fw_wrapped_exp
__host__ __device__ constexpr bool fw4_wrapped_exp(int i) {
  for (int g = 0; g < 10 * (FW4_NQB - 1) + 5; ++g)
    for (int o = 0; o < 4; ++o)
      if (fw4_sched(g, o) == (((FW4_NQB - 1) << 4) | i)) return true;
  return false;
}
// a block's row-sum adds run in the half after its row-sum MFMAs (true) or in the same half (false)
__host__ __device__ constexpr bool fw4_add_wraps(int qb) { return 10 * qb + 22 >= FW4_NG; }

__global__ __launch_bounds__(HS_NW * 64, 1) void attn_fwd_hs4_kernel(AttnArgs a, const float* knorm) {
  constexpr int NQB = FW4_NQB;
  __shared__ __attribute__((aligned(16))) char smem[HS_NSLOT * HS_SLOT_B];
  __shared__ int unsafe_wg;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = blockIdx.y, b = blockIdx.z;
  const int L = a.L;
  const int h = lane >> 5, r32 = lane & 31;
  const int qw0 = blockIdx.x * FW4_QWG + wave * (32 * NQB);
  const int nkt = (L + KT - 1) / KT;
  if (tid == 0) unsafe_wg = 0;

  // the key-norm bound over the whole key range (first: the loop runs before the Q~ fragments take their registers)
  const float* kn = knorm + ((long long)b * a.H + hh) * nkt;
  float kmax = 0.f;
  for (int t = lane; t < nkt; t += 64) kmax = fmaxf(kmax, kn[t]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) kmax = fmaxf(kmax, __shfl_xor(kmax, o));
  HS_OPAQUE(kmax);
  // Q~ = c q as B operands: lane holds q~[qw0 + 32 qb + r32][16 ks + 8h + j]; qn = ||q~|| of the lane's query
  bf16x8 qf[NQB][4];
  float qn[NQB];
  auto load_q = [&](const bf16* qp, int qb, bf16x8 (&f)[4]) __attribute__((always_inline)) {   // returns sum q~^2
    const int q = qw0 + 32 * qb + r32;
    float ss = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 t{};
      if (q < L) t = *(const bf16x8*)(qp + (long long)q * a.rs_q + 16 * ks + 8 * h);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        t[j] = to_bf16(to_f32(t[j]) * a.c);
        ss += to_f32(t[j]) * to_f32(t[j]);
      }
      f[ks] = t;
    }
    return ss;
  };
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) qn[qb] = sqrtf(wave_sum_xor32(load_q(a.q + b * a.bs_q + hh * a.hs, qb, qf[qb])));
  // the exact row max of the first key tile
  const bf16* kp = a.k + b * a.bs_k + hh * a.hs;
  const bf16* vp = a.v + b * a.bs_v + hh * a.hs;
  float m[NQB];
  {
    bf16x8 k0[2][4];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int key = 32 * kb + r32;
        k0[kb][ks] = key < L ? *(const bf16x8*)(kp + (long long)key * a.rs_k + 16 * ks + 8 * h) : bf16x8{};
      }
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      float mx = NEG_BIG;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 sc = {};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) sc = mfma32(k0[kb][ks], qf[qb][ks], sc);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (32 * kb + (i & 3) + 8 * (i >> 2) + 4 * h < L) mx = fmaxf(mx, sc[i]);
      }
      m[qb] = wave_max_xor32(mx);
    }
  }
  __syncthreads();
  {
    bool safe = true;
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) safe = safe && (qn[qb] * kmax - m[qb] <= SAFE_EXP2);
    if (!__all(safe) && lane == 0) unsafe_wg = 1;
  }
  __syncthreads();
  const int unsafe = __builtin_amdgcn_readfirstlane(unsafe_wg);

  if (unsafe) {
    // exact online softmax, 32 keys at a time (operands straight from global memory: the rare path), two query
    // blocks per sweep over the keys: four blocks' O^T beside the compiler's own operand registers would not fit
    auto sweep = [&](auto Q0) __attribute__((always_inline)) {
    constexpr int q0 = decltype(Q0)::value;
    // the sweep's own Q~ fragments, loaded again (through a pointer the compiler cannot match with the prologue's, so
    // that the other pair's fragments do not stay live through this sweep)
    const bf16* qp = a.q + b * a.bs_q + hh * a.hs;
    asm volatile("" : "+s"(qp));
    bf16x8 qf[NQB][4];
#pragma unroll
    for (int i = q0; i < q0 + 2; ++i) load_q(qp, i, qf[i]);
    f32x16 o[NQB][2];
    float mr[NQB], lr[NQB];
#pragma unroll
    for (int i = q0; i < q0 + 2; ++i) {
      mr[i] = m[i];
      lr[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) o[i][j] = f32x16{};
    }
    for (int k0 = 0; k0 < L; k0 += 32) {
      bf16x8 kr[4], vt[2][2];
      // rows past L read the last key's (no select, so no zero-initialised fragment registers): their scores are
      // replaced by NEG_BIG below, and a score depends on its own key's row only
      const int key = min(k0 + r32, L - 1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kr[ks] = *(const bf16x8*)(kp + (long long)key * a.rs_k + 16 * ks + 8 * h);
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < 8; ++j) {   // V^T: lane (h, d) holds V[key k(8h + j)][d], k-order of the P packs
            const int kk = k0 + 16 * s2 + (j & 3) + 8 * (j >> 2) + 4 * h;
            vt[db][s2][j] = kk < L ? vp[(long long)kk * a.rs_v + 32 * db + r32] : to_bf16(0.f);
          }
#pragma unroll
      for (int qb = q0; qb < q0 + 2; ++qb) {
        f32x16 sc = {};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) sc = mfma32(kr[ks], qf[qb][ks], sc);
        float mx = NEG_BIG;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (k0 + (i & 3) + 8 * (i >> 2) + 4 * h >= L) sc[i] = NEG_BIG;
          mx = fmaxf(mx, sc[i]);
        }
        const float mn = fmaxf(mr[qb], wave_max_xor32(mx));
        const float alpha = exp2_fast(mr[qb] - mn);
        mr[qb] = mn;
        lr[qb] *= alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o[qb][0][i] *= alpha; o[qb][1][i] *= alpha; }
        bf16x8 pk[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = exp2_fast(sc[i] - mn);
          lr[qb] += p;
          pk[i >> 3][i & 7] = to_bf16(p);
        }
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) o[qb][db] = mfma32(vt[db][s2], pk[s2], o[qb][db]);
      }
    }
#pragma unroll
    for (int qb = q0; qb < q0 + 2; ++qb) {
      const int q = qw0 + 32 * qb + r32;
      const float lt = wave_sum_xor32(lr[qb]);
      if (q < L) {
        const float inv = 1.f / lt;
        bf16* op = a.out + b * a.bs_out + (long long)q * a.rs_out + hh * a.hs;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            bf16x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = to_bf16(o[qb][db][4 * g + j] * inv);
            *(bf16x4*)(op + 32 * db + 8 * g + 4 * h) = w;
          }
        if (h == 0) a.lse2[((long long)b * a.H + hh) * L + q] = mr[qb] + __log2f(lt);
      }
    }
    };
    static_assert(NQB % 2 == 0, "the exact path sweeps the keys once per pair of query blocks");
#pragma unroll
    for (int q0 = 0; q0 < NQB; q0 += 2) {
      if (q0 == 0) sweep(std::integral_constant<int, 0>{});
      else sweep(std::integral_constant<int, 2>{});
    }
    return;
  }

  // ---- the placed stream
#pragma unroll
  for (int i = 0; i < NQB; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) HS_TO_AGPR(qf[i][j]);
  const int rs2k = a.rs_k * 2, rs2v = a.rs_v * 2;
  const HsRing ring = hs_ring(hs_rows_rsrc(kp, rs2k, L), rs2k, hs_rows_rsrc(vp, rs2v, L), rs2v, lane, wave, smem);
  // LDS byte offsets of every distinct fragment read within a ring slot (as attn_fwd_hs_kernel)
  unsigned row_off[2][4], tr_off[2][4][2];   // [rows 0-31 | 32-63][k-step | fragment][part]
#pragma unroll
  for (int r0i = 0; r0i < 2; ++r0i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      row_off[r0i][k] = 2 * sw128(32 * r0i + r32, 16 * k + 8 * h);
      HS_OPAQUE(row_off[r0i][k]);
#pragma unroll
      for (int part = 0; part < 2; ++part) {   // fragment k = (d block k & 1, k-step k >> 1)
        const int rw = 32 * r0i + 16 * (k >> 1) + 4 * h + ((lane & 15) >> 2) + 8 * part;
        const int col = 32 * (k & 1) + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        tr_off[r0i][k][part] = HS_TILE_B + 2 * sw128(rw, col);
        HS_OPAQUE(tr_off[r0i][k][part]);
      }
    }
  auto row = [&](int soff, int r0i, int ks) __attribute__((always_inline)) {
    return *(const bf16x8*)(smem + row_off[r0i][ks] + soff);
  };
  auto trh = [&](int soff, int r0i, int f, int part) __attribute__((always_inline)) {
    return lds_tr4((const bf16*)(smem + tr_off[r0i][f][part] + soff));
  };

  f32x16 o[NQB][2];   // [query block][d block] O^T, lane = query, rows d = 32 db + (i & 3) + 8 (i >> 2) + 4h
  f32x16 S[NQB];      // [query block] S~^T - m, then P (rows = the half's 32 keys)
  f32x16 NM[NQB];     // -m splat: the chains' initial accumulator
  u32x4 pp[NQB][2];   // [query block][k-step] bf16 P^T packs
  bf16x4 vt[2][2][2][2];   // [set][d block][k-step][half of the fragment] transposed V (keys as the k index)
  bf16x8 kr[4];       // K row fragments (A operands of the chains)
  float lp[NQB][2];   // [query block][row half] running f32 row sums (lanes 0-15: queries 16 s + lane)
  f32x4 rs[NQB];      // [query block] the half's row-sum partial on the matrix pipe: D rows 0 / 1 in lanes 0-15
  bf16x8 sel;         // 16x16x32 A operand: row 0 selects lane groups 0 / 2, row 1 groups 1 / 3 (all 8 k per lane)
  {
    const int m16 = lane & 15, g16 = lane >> 4;
    const float one = (m16 == 0 && (g16 & 1) == 0) || (m16 == 1 && (g16 & 1) == 1) ? 1.f : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sel[j] = to_bf16(one);
    HS_TO_AGPR(sel);
  }
#pragma unroll
  for (int i = 0; i < NQB; ++i) {
#pragma unroll
    for (int e = 0; e < 16; ++e) NM[i][e] = -m[i];
    HS_OPAQUE(NM[i]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      o[i][j] = f32x16{};
      HS_TO_AGPR(o[i][j]);
      pp[i][j] = u32x4{};
      HS_OPAQUE(pp[i][j]);
    }
    lp[i][0] = lp[i][1] = 0.f;
    rs[i] = f32x4{};
    HS_OPAQUE(rs[i]);
  }
  // only the last block's S is read (by its wrapped VALU) before a chain has written it
#pragma unroll
  for (int e = 0; e < 16; ++e) S[NQB - 1][e] = fw4_wrapped_exp(e) ? NEG_BIG : 0.f;
  HS_OPAQUE(S[NQB - 1]);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        vt[0][i][j][k] = vt[1][i][j][k] = bf16x4{};
        HS_OPAQUE(vt[0][i][j][k]);
        HS_OPAQUE(vt[1][i][j][k]);
      }

  auto valu_op = [&](unsigned char cd, int only_qb) __attribute__((always_inline)) {
    if (cd == 0xFF) return;
    const int kind = cd >> 6, qb = (cd >> 4) & 3, i = cd & 15;
    if (only_qb >= 0 && qb != only_qb) return;
    if (kind == 0) HS_EXP(S[qb][i]);
    else if (kind == 1) {
      asm volatile("v_add_f32 %0, %0, %1" : "+v"(lp[qb][i]) : "v"(rs[qb][i]));
      // rows 2 / 3 of the accumulator are never read, but the next MFMA writes all four registers: keep them
      // allocated so that nothing else lives in them inside its hazard window
      if (i == 1) HS_KEEP(rs[qb]);
    } else HS_CVT(pp[qb][i >> 2][i & 3], S[qb][2 * i], S[qb][2 * i + 1]);
  };
  auto pv_mfma = [&](int k, int qb, int st) __attribute__((always_inline)) {   // k: (d block k & 1, k-step k >> 1)
    const int db = k & 1, s2 = k >> 1;
    HS_MFMA_G(o[qb][db], cat44(vt[st][db][s2][0], vt[st][db][s2][1]), __builtin_bit_cast(bf16x8, pp[qb][s2]));
  };
  // the half's row-sum partial of block qb: the column sums of its two P^T packs (k-step 0 starts from zero)
  auto rs_mfma = [&](int qb, int s2) __attribute__((always_inline)) {
    if (s2 == 0)
      asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(rs[qb]) : "a"(sel), "v"(pp[qb][0]));
    else
      asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(rs[qb]) : "a"(sel), "v"(pp[qb][1]));
  };
  // gap g = 10 bq + r: r 0-3 the S chain of block bq | r 4 5 (6) 7 8 (9) PV / row sums of block bq - 1 (block 0's
  // gaps: the last block, with the previous half's V^T set)
  auto mfma_gap = [&](int g, int C, const f32x16 (&init)[NQB]) __attribute__((always_inline)) {
    const int bq = g / 10, r = g % 10;
    if (r < 4) {
      if (r == 0) HS_MFMA_C0(S[bq], kr[0], qf[bq][0], init[bq]); else HS_MFMA_C(S[bq], kr[r], qf[bq][r]);
    } else {
      const int pq = (bq + NQB - 1) % NQB;
      if (r == 6 || r == 9) rs_mfma(pq, r == 9);
      else pv_mfma(r < 6 ? r - 4 : r - 5, pq, bq == 0 ? C ^ 1 : C);
    }
  };

  // one 32-key half (rows 32 r0i of the slot at byte offset soff, V^T set SET): the transposed V fragments at gaps 0-7,
  // the next half's K rows (rows 32 nr0i of the slot at nsoff) at gaps KR0 .. KR0+3, right behind the gap's MFMA
  auto half = [&](auto SET, auto FIXED, int soff, int r0i, int nsoff, int nr0i, const f32x16 (&init)[NQB], auto hook)
      __attribute__((always_inline)) {
    constexpr int C = decltype(SET)::value;
    constexpr bool FIXED_SLOT = decltype(FIXED)::value;
    constexpr int NG = FW4_NG;
    constexpr int KR0 = 10 * (NQB - 1) + 3;   // each fragment reloaded 3 gaps after the last chain's read of it
    auto lds_reads = [&](int g) __attribute__((always_inline)) {
      if (g < 8) {
        const int f = g >> 1, part = g & 1;   // fragment f = (d block f & 1, k-step f >> 1)
        vt[C][f & 1][f >> 1][part] = trh(soff, r0i, f, part);
      } else if (g >= KR0 && g < KR0 + 4) {   // the next half's K rows
        kr[g - KR0] = row(nsoff, nr0i, g - KR0);
      }
    };
    // (unrolled by pack expansion: 40 gaps of this size are past the loop unroller's limit for `#pragma unroll`)
    hs_for_gaps([&](auto G) __attribute__((always_inline)) {
      constexpr int g = decltype(G)::value;
      mfma_gap(g, C, init);
      if (g % 10 == 2) HS_KEEP(init[g / 10]);   // the chain-start MFMAs read their initial accumulators as SrcC after issue
      lds_reads(g);
      // run-time-slot tiles (remainder, ragged last tile): the compiler may sink their LDS reads, so the wait states
      // between a chain's last MFMA and its first exp are padded explicitly
      if (!FIXED_SLOT && g % 10 == 5) asm volatile("s_nop 1" ::: "memory");
      // a first-exp gap with no LDS read behind its MFMA: the wait state the read gives elsewhere
      if (g % 10 == 5 && g >= 8 && !(g >= KR0 && g < KR0 + 4)) asm volatile("s_nop 0" ::: "memory");
      valu_op(fw4_sched(g, 0), -1);
      valu_op(fw4_sched(g, 1), -1);
      valu_op(fw4_sched(g, 2), -1);
      valu_op(fw4_sched(g, 3), -1);
      hook(g);
    }, std::make_integer_sequence<int, NG>{});
  };

  // register staging as attn_fwd_hs_kernel: tile t+1's pieces are stored to ring slot (t+1) & 3 at gaps 1-7 of tile
  // t's half 0 and tile t+2's loaded at gaps 11-17; the barrier at gap 7 of tile t's half 1 publishes tile t+1 (first
  // reader: the K rows at gaps KR0 ..)
  u32x4 stg[4];
  const unsigned wst = ring.lds0 + 2048 * wave + 16 * lane;
  auto ld_piece = [&](int t, int i) __attribute__((always_inline)) {
    stg[i] = hs_ld16(ring.rsrc(i), ring.voff(i), ring.soff(t, i));
  };
  // prologue: tile 0 by LDS-DMA, tile 1 into the staging AGPRs; wait for tile 0; K rows of its first half
  ring.dma(0, 0); ring.dma(0, 1); ring.dma(0, 2); ring.dma(0, 3);
  ld_piece(1, 0); ld_piece(1, 1); ld_piece(1, 2); ld_piece(1, 3);
  hs_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kr[ks] = row(0, 0, ks);
  __builtin_amdgcn_s_waitcnt(LGKM0_WAIT);

  // SL >= 0: tile t sits in ring slot SL (compile-time: immediates); SL < 0: slot t & 3 at run time. ia / ib: the
  // chains' initial accumulators of half 0 / 1; mid() runs between the halves
  auto tile = [&](auto SL, int t, const f32x16 (&ia)[NQB], const f32x16 (&ib)[NQB], auto mid)
      __attribute__((always_inline)) {
    constexpr int sl = decltype(SL)::value;
    const int soff = sl >= 0 ? sl * HS_SLOT_B : (t & (HS_NSLOT - 1)) * HS_SLOT_B;
    const int nsoff = sl >= 0 ? ((sl + 1) & (HS_NSLOT - 1)) * HS_SLOT_B : ((t + 1) & (HS_NSLOT - 1)) * HS_SLOT_B;
    auto stage = [&](int g) __attribute__((always_inline)) {
      if (t + 1 < nkt && g == 7) __builtin_amdgcn_s_barrier();
    };
    constexpr int LD0 = 11;   // tile t+2's loads at gaps 11, 13, 15, 17 (32x32x16 gaps)
    auto rstg = [&](int g) __attribute__((always_inline)) {
      if (g == 1) hs_vmcnt<0>();   // tile t+1's pieces (loaded a tile ago)
      if (g < 8 && (g & 1)) {
        constexpr int S1 = sl >= 0 ? ((sl + 1) & (HS_NSLOT - 1)) * HS_SLOT_B : 0;
        const unsigned base = sl >= 0 ? wst : wst + (unsigned)(((t + 1) & (HS_NSLOT - 1)) * HS_SLOT_B);
        switch (g) {
          case 1: hs_st16<S1>(base, stg[0]); break;
          case 3: hs_st16<S1 + 1024>(base, stg[1]); break;
          case 5: hs_st16<S1 + HS_TILE_B>(base, stg[2]); break;
          default: hs_st16<S1 + HS_TILE_B + 1024>(base, stg[3]); break;
        }
      } else if (g >= LD0 && g < LD0 + 8 && ((g - LD0) & 1) == 0) {
        ld_piece(t + 2, (g - LD0) >> 1);
      }
    };
    half(std::integral_constant<int, 0>{}, std::bool_constant<(sl >= 0)>{}, soff, 0, soff, 1, ia, rstg);
    mid();
    half(std::integral_constant<int, 1>{}, std::bool_constant<(sl >= 0)>{}, soff, 1, nsoff, 0, ib, stage);
  };
  const bool ragged = (L & (KT - 1)) != 0;
  const int nfast = ragged ? nkt - 1 : nkt;
  using IC0 = std::integral_constant<int, 0>;
  using IC1 = std::integral_constant<int, 1>;
  using IC2 = std::integral_constant<int, 2>;
  using IC3 = std::integral_constant<int, 3>;
  using ICR = std::integral_constant<int, -1>;
  auto nop = [] {};
  int t = 0;
  for (; t + 4 <= nfast; t += 4) {   // t & 3 == 0 here
    tile(IC0{}, t, NM, NM, nop);
    tile(IC1{}, t + 1, NM, NM, nop);
    tile(IC2{}, t + 2, NM, NM, nop);
    tile(IC3{}, t + 3, NM, NM, nop);
  }
  for (; t < nfast; ++t) tile(ICR{}, t, NM, NM, nop);
  if (ragged) {   // the last tile: keys past L start from NEG_BIG (their K rows read as zero), so exp2 gives 0
    const int tl = nkt - 1;
    // one half's initial accumulators at a time (four blocks of both halves would not fit beside the stream); the
    // second half's are written between the halves, long after the first half's chain starts read theirs
    f32x16 M[NQB];
    auto mk = [&](int hf) __attribute__((always_inline)) {
      int Lo = L;
      asm volatile("" : "+s"(Lo));   // (not before the stream so far)
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          M[qb][e] = tl * KT + 32 * hf + (e & 3) + 8 * (e >> 2) + 4 * h < Lo ? -m[qb] : NEG_BIG;
        HS_OPAQUE(M[qb]);
      }
      asm volatile("s_nop 4" ::: "memory");
    };
    mk(0);
    tile(ICR{}, tl, M, M, [&]() __attribute__((always_inline)) { mk(1); });
  }
  hs_vmcnt<0>();   // the last tiles' staging loads (past the end: zeros) retire before the exit
  // the last query block of the last half: its wrapped VALU and its PV (and row-sum) MFMAs
#pragma unroll
  for (int g = 0; g < 10; ++g) {
#pragma unroll
    for (int op = 0; op < 4; ++op) valu_op(fw4_sched(g, op), NQB - 1);
    if (g >= 4) {
      asm volatile("s_nop 1" ::: "memory");
      if (g == 6 || g == 9) rs_mfma(NQB - 1, g == 9);
      else pv_mfma(g < 6 ? g - 4 : g - 5, NQB - 1, 1);   // the last half is a half 1
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) HS_OPAQUE(rs[qb]);   // read only after the last MFMAs completed

#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int q = qw0 + 32 * qb + r32;
    // l of query 16 s + n sits in lane n, row s of the block's 16x16 accumulator (+ the last half's partials where
    // the stream has not added them yet)
    const float s0 = fw4_add_wraps(qb) ? lp[qb][0] + rs[qb][0] : lp[qb][0];
    const float s1 = fw4_add_wraps(qb) ? lp[qb][1] + rs[qb][1] : lp[qb][1];
    const float l0 = __shfl(s0, r32 & 15), l1 = __shfl(s1, r32 & 15);
    const float lt = r32 < 16 ? l0 : l1;
    if (q < L) {
      const float inv = 1.f / lt;
      bf16* op = a.out + b * a.bs_out + (long long)q * a.rs_out + hh * a.hs;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = to_bf16(o[qb][db][4 * g + j] * inv);
          *(bf16x4*)(op + 32 * db + 8 * g + 4 * h) = w;
        }
      if (h == 0) a.lse2[((long long)b * a.H + hh) * L + q] = m[qb] + __log2f(lt);
    }
  }
}

}  // namespace lci

// =============================================================================== C-ABI entry points
using namespace lci;

static int check_packed(const void* p, int rs) {
  return ((uintptr_t)p % 16 == 0) && (rs % 8 == 0);
}

// The checks lci_attn_fwd* and lci_attn_bwd* share (`what` names the entry point in the messages): head dim, shape,
// alignment of the packed qkv-layout tensors (qkv; dqkv in the backward) and of the (B, L, H*64) ones (out; dout), and
// the 32-bit range of the placed kernels' buffer offsets. They address rows through buffer resources with 32-bit
// sizes and stage key tiles up to two past the tile count padded to a multiple of 4: rows below L + 6 KT.
static int attn_check(const char* what, const void* qkv, const void* dqkv, const void* out, const void* dout, int B,
                      int L, int H, int head_dim) {
  LCI_CHECK(head_dim == DH, "%s: head_dim %d unsupported (only 64)", what, head_dim);
  LCI_CHECK(B > 0 && L > 0 && H > 0, "%s: bad shape B=%d L=%d H=%d", what, B, L, H);
  const int rs = 3 * H * DH;
  LCI_CHECK(check_packed(qkv, rs) && (!dqkv || check_packed(dqkv, rs)) && check_packed(out, H * DH) &&
                (!dout || check_packed(dout, H * DH)), "%s: misaligned pointers", what);
  LCI_CHECK((long long)(L + 6 * KT) * rs * 2 < (1ll << 31), "%s: L=%d too long for 32-bit buffer offsets", what, L);
  return 0;
}

// The AttnArgs fields forward and backward share: q | k | v inside the packed qkv (B, L, 3*H*64), shape and scales
static AttnArgs attn_args(const void* qkv, int L, int H, float scale) {
  AttnArgs a{};
  const int rs = 3 * H * DH;
  const bf16* base = (const bf16*)qkv;
  a.q = base; a.k = base + H * DH; a.v = base + 2 * H * DH;
  a.bs_q = a.bs_k = a.bs_v = (long long)L * rs;
  a.rs_q = a.rs_k = a.rs_v = rs;
  a.hs = DH; a.H = H; a.L = L;
  a.scale = scale; a.c = scale * 1.4426950408889634f;
  return a;
}

extern "C" long long lci_attn_fwd_ws_bytes(int B, int L, int H) {
  return (long long)B * H * ((L + KT - 1) / KT) * sizeof(float);
}

// Which forward kernel serves a shape (0 = attn_fwd_hs_kernel, 1 = attn_fwd_hs4_kernel): the wide kernel only where
// its grid of W workgroups both fills the chip and leaves no worse a tail than the narrow one's, i.e. W >= n_cu and
// W / (ceil(W / n_cu) n_cu) >= 0.9. Pure host arithmetic (no device needed).
static int attn_wide_pick(int B, int L, int H, int n_cu, int qwg) {   // qwg: queries per wide workgroup
  if (B <= 0 || L <= 0 || H <= 0 || n_cu <= 0) return 0;
  const long long W = (long long)B * H * ((L + qwg - 1) / qwg);
  if (W < n_cu) return 0;
  const long long rounds = (W + n_cu - 1) / n_cu;
  return 10 * W >= 9 * rounds * n_cu ? 1 : 0;
}
extern "C" int lci_attn_fwd_pick(int B, int L, int H, int n_cu) { return attn_wide_pick(B, L, H, n_cu, FW4_QWG); }
// The same rule for the dQ kernel of the backward (0 = attn_bwd_dq_hs_kernel, 1 = attn_bwd_dq_hs4_kernel)
extern "C" int lci_attn_bwd_dq_pick(int B, int L, int H, int n_cu) { return attn_wide_pick(B, L, H, n_cu, DQ4_QWG); }

static int attn_n_cu() {   // compute units of the current device, asked once per process
  static const int n = [] {
    int dev = 0, cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 0;
    return cu;
  }();
  return n;
}

// variant: -1 = lci_attn_fwd_pick, 0 = attn_fwd_hs_kernel, 1 = attn_fwd_hs4_kernel (for tests and A/B timing)
extern "C" int lci_attn_fwd_variant(int variant, const void* qkv, void* out, float* lse2, float* knorm_ws, int B,
                                    int L, int H, int head_dim, float scale, void* stream) {
  LCI_CHECK(variant >= -1 && variant <= 1, "lci_attn_fwd_variant: variant %d (want -1, 0 or 1)", variant);
  if (attn_check("lci_attn_fwd", qkv, nullptr, out, nullptr, B, L, H, head_dim)) return 1;
  LCI_CHECK(knorm_ws != nullptr, "lci_attn_fwd: knorm_ws (lci_attn_fwd_ws_bytes) is required");
  AttnArgs a = attn_args(qkv, L, H, scale);
  a.out = (bf16*)out; a.lse2 = lse2;
  a.bs_out = (long long)L * H * DH; a.rs_out = H * DH;
  hipStream_t s = (hipStream_t)stream;
  const int nkt = (L + KT - 1) / KT;
  hipLaunchKernelGGL(attn_key_norm_kernel, dim3((nkt + 3) / 4, H, B), dim3(256), 0, s, a, knorm_ws, nkt);
  LCI_LAUNCH_CHECK();
  if (variant < 0) variant = lci_attn_fwd_pick(B, L, H, attn_n_cu());
  if (variant == 1)
    hipLaunchKernelGGL(attn_fwd_hs4_kernel, dim3((L + FW4_QWG - 1) / FW4_QWG, H, B), dim3(HS_NW * 64), 0, s, a,
                       (const float*)knorm_ws);
  else
    hipLaunchKernelGGL(attn_fwd_hs_kernel, dim3((L + HS_NW * 64 - 1) / (HS_NW * 64), H, B), dim3(HS_NW * 64), 0, s, a,
                       (const float*)knorm_ws);
  LCI_LAUNCH_CHECK();
  return 0;
}

extern "C" int lci_attn_fwd(const void* qkv, void* out, float* lse2, float* knorm_ws, int B, int L, int H,
                            int head_dim, float scale, void* stream) {
  return lci_attn_fwd_variant(-1, qkv, out, lse2, knorm_ws, B, L, H, head_dim, scale, stream);
}

// backward workspace: (B, H, 2, L) f32 negated row constants [-lse2 | -delta], then the wide dQ kernel's int32 flags
// [B][H][ceil(L / 512)] (dq4_flag_offset), 256-B aligned
extern "C" long long lci_attn_bwd_ws_bytes(int B, int H, int L) {
  const long long flags = (long long)B * H * ((L + DQ4_QWG - 1) / DQ4_QWG);
  return ((dq4_flag_offset(B, H, L) + flags) * 4 + 255) / 256 * 256;
}

// How lci_attn_bwd splits the keys of the dK/dV pass: the number W of attn_bwd_dkdv_hs3_kernel workgroups (384 keys
// each, keys [0, 384 W)) per (batch, head); attn_bwd_dkdv_hs_kernel takes the keys from 384 W on. 0 = the narrow
// kernel alone. A split qualifies when both grids pass attn_wide_pick's rule (at least n_cu workgroups and >= 0.9 of
// the rounds they occupy; the narrow grid may also be empty). A wide workgroup does 1.5 narrow workgroups' work, so
// a split costs 3 rounds_wide + 2 rounds_narrow against 2 rounds of the narrow kernel alone: the cheapest qualifying
// split is taken (the larger W on a tie) if it costs no more than the narrow kernel alone. Pure host arithmetic.
// The metric shape (B H = 12, L = 65536, 256 CUs): W = 128, 6 wide + 3 narrow rounds; L = 16384 and 32768: 0.
// (DESIGN.md "Attention backward dK/dV: 96 keys per wave on a split key grid" has the measurements.)
static bool attn_grid_fills(long long wgs, int n_cu) {
  return wgs >= n_cu && 10 * wgs >= 9 * ((wgs + n_cu - 1) / n_cu) * n_cu;
}
extern "C" int lci_attn_bwd_dkdv_pick(int B, int L, int H, int n_cu) {
  if (B <= 0 || L <= 0 || H <= 0 || n_cu <= 0) return 0;
  const long long bh = (long long)B * H;
  const int nkw = HS_NW * 64;
  long long best_cost = 2 * ((bh * ((L + nkw - 1) / nkw) + n_cu - 1) / n_cu);
  int best = 0;
  for (int W = 1; W <= L / DKV3_KWG; ++W) {
    const long long wide = bh * W, rest = bh * ((L - DKV3_KWG * W + nkw - 1) / nkw);
    if (!attn_grid_fills(wide, n_cu) || (rest && !attn_grid_fills(rest, n_cu))) continue;
    const long long cost = 3 * ((wide + n_cu - 1) / n_cu) + 2 * ((rest + n_cu - 1) / n_cu);
    if (cost <= best_cost) best_cost = cost, best = W;
  }
  return best;
}

// dq_variant: -1 = lci_attn_bwd_dq_pick, 0 = attn_bwd_dq_hs_kernel, 1 = attn_bwd_dq_hs4_kernel + its fallback launch;
// dkdv_wide_wgs: -1 = lci_attn_bwd_dkdv_pick, 0 = attn_bwd_dkdv_hs_kernel alone, W > 0 = attn_bwd_dkdv_hs3_kernel on
// keys [0, 384 W) (384 (W - 1) < L) and the narrow kernel on the rest;
// stage: -1 = all launches; 0 = delta, 1 = dK/dV, 2 = dQ (for per-kernel timing)
extern "C" int lci_attn_bwd_variant2(int dq_variant, int dkdv_wide_wgs, int stage, const void* qkv, const void* out,
                                     const void* dout, const float* lse2, void* dqkv, float* delta_ws, int B, int L,
                                     int H, int head_dim, float scale, void* stream) {
  LCI_CHECK(dq_variant >= -1 && dq_variant <= 1, "lci_attn_bwd_variant: dq_variant %d (want -1, 0 or 1)", dq_variant);
  if (attn_check("lci_attn_bwd", qkv, dqkv, out, dout, B, L, H, head_dim)) return 1;
  LCI_CHECK(dkdv_wide_wgs >= -1 && (dkdv_wide_wgs <= 0 || (long long)DKV3_KWG * (dkdv_wide_wgs - 1) < L),
            "lci_attn_bwd_variant2: dkdv_wide_wgs %d (want -1, 0 or at most ceil(L / 384) = %d)", dkdv_wide_wgs,
            (L + DKV3_KWG - 1) / DKV3_KWG);
  LCI_CHECK(delta_ws != nullptr, "lci_attn_bwd: delta_ws (lci_attn_bwd_ws_bytes) is required");
  AttnArgs a = attn_args(qkv, L, H, scale);
  bf16* dbase = (bf16*)dqkv;
  a.o = (const bf16*)out; a.dout = (const bf16*)dout;
  a.lse2 = (float*)lse2; a.delta = delta_ws;
  a.bs_o = a.bs_do = (long long)L * H * DH;
  a.rs_o = a.rs_do = H * DH;
  a.out = dbase; a.dk = dbase + H * DH; a.dv = dbase + 2 * H * DH;
  a.bs_out = a.bs_dk = a.bs_dv = a.bs_q;
  a.rs_out = a.rs_dk = a.rs_dv = a.rs_q;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((L + HS_NW * 64 - 1) / (HS_NW * 64), H, B);
  if (stage < 0 || stage == 0) {
    hipLaunchKernelGGL(attn_bwd_delta_kernel, dim3((L + 31) / 32, H, B), dim3(256), 0, s, a);
    LCI_LAUNCH_CHECK();
  }
  if (stage < 0 || stage == 1) {
    const int W = dkdv_wide_wgs < 0 ? lci_attn_bwd_dkdv_pick(B, L, H, attn_n_cu()) : dkdv_wide_wgs;
    if (W > 0) {
      hipLaunchKernelGGL(attn_bwd_dkdv_hs3_kernel, dim3(W, H, B), dim3(HS_NW * 64), 0, s, a);
      LCI_LAUNCH_CHECK();
    }
    a.k0 = W * DKV3_KWG;   // the narrow kernel's first key
    if (a.k0 < L) {
      hipLaunchKernelGGL(attn_bwd_dkdv_hs_kernel, dim3((L - a.k0 + HS_NW * 64 - 1) / (HS_NW * 64), H, B),
                         dim3(HS_NW * 64), 0, s, a);
      LCI_LAUNCH_CHECK();
    }
  }
  if (stage < 0 || stage == 2) {
    if (dq_variant < 0) dq_variant = lci_attn_bwd_dq_pick(B, L, H, attn_n_cu());
    if (dq_variant == 1) {
      // the wide kernel, then the narrow stream for the workgroups it flagged (none: a few microseconds)
      hipLaunchKernelGGL(attn_bwd_dq_hs4_kernel, dim3((L + DQ4_QWG - 1) / DQ4_QWG, H, B), dim3(HS_NW * 64), 0, s, a);
      LCI_LAUNCH_CHECK();
      hipLaunchKernelGGL(attn_bwd_dq_hsfb_kernel, grid, dim3(HS_NW * 64), 0, s, a);
    } else {
      hipLaunchKernelGGL(attn_bwd_dq_hs_kernel, grid, dim3(HS_NW * 64), 0, s, a);
    }
    LCI_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int lci_attn_bwd_variant(int dq_variant, int stage, const void* qkv, const void* out, const void* dout,
                                    const float* lse2, void* dqkv, float* delta_ws, int B, int L, int H, int head_dim,
                                    float scale, void* stream) {
  return lci_attn_bwd_variant2(dq_variant, -1, stage, qkv, out, dout, lse2, dqkv, delta_ws, B, L, H, head_dim, scale,
                               stream);
}

extern "C" int lci_attn_bwd_stage(int stage, const void* qkv, const void* out, const void* dout, const float* lse2,
                                  void* dqkv, float* delta_ws, int B, int L, int H, int head_dim, float scale,
                                  void* stream) {
  return lci_attn_bwd_variant(-1, stage, qkv, out, dout, lse2, dqkv, delta_ws, B, L, H, head_dim, scale, stream);
}

extern "C" int lci_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse2, void* dqkv,
                            float* delta_ws, int B, int L, int H, int head_dim, float scale, void* stream) {
  return lci_attn_bwd_stage(-1, qkv, out, dout, lse2, dqkv, delta_ws, B, L, H, head_dim, scale, stream);
}
