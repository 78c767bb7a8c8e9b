// Swin shifted-window attention for LARGE windows (grid mode, head_dim 32, up to 4096 tokens per window) on gfx950.
//
// window.hip keeps a whole window's K and V in LDS and reads the additive logit term from an N^2-sized table; that
// stops at 768 tokens. The kernels here stream 32-key (or 32-query) tiles through LDS flash-style and evaluate the
// additive term per pair in the kernel, so nothing they build grows as N^2 per launch except the bounded dS chunk of
// the table gradient (below). The pad / roll / partition row map, the window type and the region ids are win_row /
// win_type / win_region of window_geo.hpp: the functions the resident kernels use.
//
// Logit of a pair, log2 domain:
//     s = fma(qk, c, t)     qk = sum_d q[d] k[d]  bf16 x bf16 products, f32 accumulation (two 32x32x16 MFMAs; q and k
//                                are the bf16 qkv values as stored: no prescaled, re-rounded operand),
//                           c  = fl(scale * log2(e)),
//                           t  = fl(table[rel(q, k)][h] * log2(e))            (one f32 rounding),
//                           t  = fl(t + fl(-100 * log2(e)))  if region(q) != region(k)   (one more),
//                           s  = -1e30 for a key (or query) beyond the window's N tokens.
// The fma rounds once. rel(q, k) = code(q) - code(k) + c0 with code(n) = sum_s coord_s(n) * W_s, W_s =
// prod_{t>s} (2 fw_t - 1), c0 = sum_s (fw_s - 1) W_s, the coordinates decoded from the raster of the module's FULL
// window fw (token j of a clamped window is raster position j of the full one: relative_position_index[:n, :n]).
// code < 2^15 and the region id (< 27) share one int per token, built once per workgroup in LDS beside the row map.
// Table: one head's column of the module's (n_tab, H) f32 parameter, multiplied by log2(e) once and staged in LDS as
// f32 when it has at most 16384 rows (64 KB: every 2-D window up to 64 x 64 = 16129 rows and 3-D up to 12^3); larger
// tables (16^3: 29791 rows = 119 KB) are read through the cache from global memory and multiplied at use. Both paths
// take the same f32 values through the same single rounding, so they agree bit for bit.
// Softmax: online over 32-key tiles with the lazy exact rescale of window.hip; P = exp2(s - m) in f32 (v_exp_f32),
// rounded to bf16 as the operand of O += V^T P^T; l and O accumulate in f32; out = bf16(O / l), lse2 = m + log2(l).
//
// Forward:  one workgroup = 128 queries (4 waves x 32, the query on the MFMA lane) of one (window, head); K and V
//           tiles of 32 keys double-buffered in LDS, one barrier per tile; S^T = K Q^T, O^T += V^T P^T.
// Backward: every kernel recomputes s by the chain above (as attention_gen.hip does).
//   wl_dq_kernel   (query on lane, K / V tiles streamed): delta = rowsum(dO * O) (also written for the next kernel),
//                  P = exp2(s - lse2), dP^T = V dO^T - delta, dS = P * dP (bf16 operand), dQ^T += K^T dS^T; optionally
//                  writes dS (bf16) for a chunk of (window, head) items into the workspace.
//   wl_dkv_kernel  (key on lane, Q / dO tiles and their lse2 / -delta streamed): dV^T += dO^T P, dK^T += Q^T dS; the
//                  padded keys' dK | dV of a workgroup are summed in a fixed order into one partial, and
//                  wl_pad_reduce_kernel adds the partials of all workgroups in a fixed order (the qkv-bias gradient).
//   Table gradient dT[r][h] = sum over windows and pairs with rel(q, k) = r of dS: no float atomics. The host walks
//                  the (window, head) items in chunks whose dS (item = N x Npad bf16) fits the workspace budget
//                  (LCI_WIN_LONG_WS_MB, default 256); per chunk wl_dq_kernel writes dS (one item = [key tile][query]
//                  [32 keys]: a wave stores its 32 x 32 tile as 2 KB of consecutive bytes) and wl_dtab_kernel, one
//                  thread per (r, range of raster rows, head), walks the chunk's items of its head in order, reads
//                  dS[q][q - D(r)] (neighbouring r = neighbouring k: coalesced; every dS element is read exactly
//                  once) and carries its f32 sum from chunk to chunk in a (range, r, h) partial array (at most 32
//                  ranges); lci::ordered_sum adds the ranges at the end. The launch list depends on the geometry and
//                  the budget only, and the result does not depend on the budget.
#include "window_geo.hpp"

#include <algorithm>

namespace lci {

constexpr int WL_MAXN = 4096;        // tokens per window
constexpr int WL_MAXTAB = 29791;     // rows of the relative-position table (16^3 window)
constexpr int WL_TAB_LDS = 16384;    // rows staged in LDS as f32
constexpr int WL_NW = 4;             // waves per workgroup: 128 queries (keys) of one (window, head)
constexpr int WL_TILE = 32 * WLD;    // elements of one staged 32-row tile
constexpr int WL_INVALID = (int)0x80000000u;   // meta of a token beyond N

struct WinLongArgs {
  WinArgs g;
  const float* table;    // (n_tab, H) f32
  float* delta;          // (Bw, H, N) f32
  bf16* ds;              // (items of the chunk, Npad / 32 key tiles, N, 32) bf16 or null
  float* part;           // (nrg, n_tab, H) f32 running table-gradient partials
  float* pad_part;       // (Bw * H * nkc, 64) f32 padded-key dK | dV partials or null
  int fw[3], wgt[3], c0, ntab;
  int i0, ni;            // first (window, head) item of this launch and their number (item = w * H + h)
  int nqc;               // 128-token chunks per window
  int rpr, nrg;          // wl_dtab_kernel: raster rows per range, ranges
};

// sum_s coord_s(n) * W_s of raster position n of the full window
__device__ __forceinline__ int wl_code(const WinLongArgs& a, int n) {
  int c = 0;
  for (int s = a.g.nd - 1; s >= 0; --s) { c += (n % a.fw[s]) * a.wgt[s]; n /= a.fw[s]; }
  return c;
}

struct WlLds {
  const bf16* bias;   // the head's q | k | v bias as bf16 (3 x 32)
  int* row;           // token row, -1 padded voxel, -2 beyond N
  int* meta;          // code | region << 16, WL_INVALID beyond N
  bf16* tile;         // [buffer 2][tensor 2][32][WLD]
  float* rc;          // [buffer 2][lse2 | -delta][32] (wl_dkv_kernel)
  float* tab;         // the head's table * log2(e) (TABL)
};

static size_t wl_lds_bytes(const WinLongArgs& a, bool tabl) {
  return 256 + (size_t)a.g.Npad * 8 + 4 * WL_TILE * 2 + 512 + (tabl ? (size_t)a.ntab * 4 : 0);
}

template <bool TABL>
__device__ __forceinline__ void wl_setup(const WinLongArgs& a, char* smem, WlLds& L, int w, int hh) {
  const WinArgs& g = a.g;
  bf16* bl = (bf16*)smem;
  L.bias = bl;
  L.row = (int*)(smem + 256);
  L.meta = L.row + g.Npad;
  L.tile = (bf16*)(L.meta + g.Npad);
  L.rc = (float*)(L.tile + 4 * WL_TILE);
  L.tab = L.rc + 128;
  const int t = win_type(g, w);
  for (int n = threadIdx.x; n < g.Npad; n += blockDim.x) {
    int rid = 0, row = -2, meta = WL_INVALID;
    if (n < g.N) {
      row = win_row(g, w, n, rid);
      meta = wl_code(a, n) | (win_region(g, t, n) << 16);
    }
    L.row[n] = row;
    L.meta[n] = meta;
  }
  if (threadIdx.x < 3 * WHD)
    bl[threadIdx.x] = to_bf16(g.qkv_bias ? g.qkv_bias[(threadIdx.x / WHD) * g.C + hh * WHD + threadIdx.x % WHD] : 0.f);
  if constexpr (TABL)
    for (int i = threadIdx.x; i < a.ntab; i += blockDim.x) L.tab[i] = a.table[(long long)i * g.H + hh] * WLOG2E;
  __syncthreads();
}

// 8 channels (16 B) at offset ch8 of the head's q (which 0) | k (1) | v (2) block of a token: the qkv row, the bias for
// a padded voxel, zeros beyond N
__device__ __forceinline__ bf16x8 wl_load8(const WinArgs& g, const WlLds& L, int row, int which, int hh, int ch8) {
  if (row >= 0) return *(const bf16x8*)(g.qkv + (long long)row * 3 * g.C + which * g.C + hh * WHD + ch8);
  if (row == -1) return *(const bf16x8*)(L.bias + which * WHD + ch8);
  return bf16x8{};
}

// 8 channels of a C-channel row (out / dout) of a token; zeros for padded voxels (cropped) and beyond N
__device__ __forceinline__ bf16x8 wl_load8_out(const WinArgs& g, const bf16* base, int row, int hh, int ch8) {
  if (row >= 0) return *(const bf16x8*)(base + (long long)row * g.C + hh * WHD + ch8);
  return bf16x8{};
}

// the additive logit term t of the header for this lane's token against a token with meta m. KEYLANE: the lane holds
// the key (base = c0 - code(key)), else the query (base = code(query) + c0); rself = the lane's region id
template <bool KEYLANE, bool TABL>
__device__ __forceinline__ float wl_term(const WinLongArgs& a, const WlLds& L, int hh, int base, int rself, int m) {
  const int code = m & 0xffff;
  const int idx = KEYLANE ? base + code : base - code;
  float t;
  if constexpr (TABL) t = L.tab[idx];
  else t = a.table[(long long)idx * a.g.H + hh] * WLOG2E;
  if (((m >> 16) & 31) != rself) t += -100.f * WLOG2E;
  return m < 0 ? WNEG : t;
}

// s[i] = fma(s[i], c, t(lane token, token tile0 + (i&3) + 8(i>>2) + 4 half))
template <bool KEYLANE, bool TABL>
__device__ __forceinline__ void wl_logits(const WinLongArgs& a, const WlLds& L, int hh, int base, int rself, int tile0,
                                          int half, f32x16& s) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int4 m4 = *(const int4*)(L.meta + tile0 + 8 * g4 + 4 * half);
    s[4 * g4 + 0] = fmaf(s[4 * g4 + 0], a.g.c, wl_term<KEYLANE, TABL>(a, L, hh, base, rself, m4.x));
    s[4 * g4 + 1] = fmaf(s[4 * g4 + 1], a.g.c, wl_term<KEYLANE, TABL>(a, L, hh, base, rself, m4.y));
    s[4 * g4 + 2] = fmaf(s[4 * g4 + 2], a.g.c, wl_term<KEYLANE, TABL>(a, L, hh, base, rself, m4.z));
    s[4 * g4 + 3] = fmaf(s[4 * g4 + 3], a.g.c, wl_term<KEYLANE, TABL>(a, L, hh, base, rself, m4.w));
  }
}

// (window, head, 128-token chunk) of workgroup blockIdx.x: the chunks of one (window, head) are neighbours
__device__ __forceinline__ void wl_item(const WinLongArgs& a, int& w, int& hh, int& chunk) {
  const int b = blockIdx.x;
  chunk = b % a.nqc;
  const int item = a.i0 + b / a.nqc;
  w = item / a.g.H;
  hh = item % a.g.H;
}

// This thread's 16-byte chunk of the K | V tile `kt` (threads 0-127: K, 128-255: V; 32 rows x 4 chunks each)
__device__ __forceinline__ bf16x8 wl_ld_kv(const WinArgs& g, const WlLds& L, int hh, int kt) {
  const int t = threadIdx.x & 127;
  return wl_load8(g, L, L.row[kt * 32 + (t >> 2)], 1 + (threadIdx.x >> 7), hh, (t & 3) * 8);
}
__device__ __forceinline__ void wl_st_tile(const WlLds& L, int buf, bf16x8 v) {
  const int t = threadIdx.x & 127;
  *(bf16x8*)(L.tile + (buf * 2 + (threadIdx.x >> 7)) * WL_TILE + (t >> 2) * WLD + (t & 3) * 8) = v;
}

// --------------------------------------------------------------------------------------------- forward
template <bool TABL>
__global__ __launch_bounds__(WL_NW * 64) void wl_fwd_kernel(WinLongArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WinArgs& g = a.g;
  int w, hh, qc;
  wl_item(a, w, hh, qc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  WlLds L;
  wl_setup<TABL>(a, smem, L, w, hh);
  const int q = (qc * WL_NW + wave) * 32 + (lane & 31);
  const bool qv = q < g.N;
  const bool active = (qc * WL_NW + wave) * 32 < g.N;   // wave-uniform: the wave has a query
  const int qrow = qv ? L.row[q] : -2;
  const int qm = qv ? L.meta[q] : 0;
  const int base = (qm & 0xffff) + a.c0, rq = (qm >> 16) & 31;
  bf16x8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = wl_load8(g, L, qrow, 0, hh, ks * 16 + 8 * half);
  wl_st_tile(L, 0, wl_ld_kv(g, L, hh, 0));
  __syncthreads();
  f32x16 o = {};
  float m = 0.f, l = 0.f;
  for (int kt = 0; kt < g.nkt; ++kt) {
    const bf16* Kt = L.tile + (kt & 1) * 2 * WL_TILE;
    const bf16* Vt = Kt + WL_TILE;
    bf16x8 nxt;
    if (kt + 1 < g.nkt) nxt = wl_ld_kv(g, L, hh, kt + 1);
    if (active) {
      f32x16 s = mfma32(frag_row(Kt, WLD, 0, 0, lane), qf[0], f32x16{});
      s = mfma32(frag_row(Kt, WLD, 0, 16, lane), qf[1], s);
      wl_logits<false, TABL>(a, L, hh, base, rq, kt * 32, half, s);
      float mx = s[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
      mx = wave_max_xor32(mx);
      if (kt == 0 || __any(mx > m)) {   // lazy exact rescale (alpha == 1 otherwise)
        const float mn = kt == 0 ? mx : fmaxf(m, mx);
        if (kt != 0) {
          const float al = exp2_fast(m - mn);
          l *= al;
#pragma unroll
          for (int i = 0; i < 16; ++i) o[i] *= al;
        }
        m = mn;
      }
      float l4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = exp2_fast(s[i] - m);
        l4[i & 3] += s[i];
      }
      l += (l4[0] + l4[1]) + (l4[2] + l4[3]);
      o = mfma32(frag_tr<0>(Vt, WLD, 0, 0, lane), pack8<0>(s), o);
      o = mfma32(frag_tr<1>(Vt, WLD, 0, 0, lane), pack8<1>(s), o);
    }
    if (kt + 1 < g.nkt) wl_st_tile(L, (kt + 1) & 1, nxt);
    __syncthreads();
  }
  const float lt = wave_sum_xor32(l);
  const float inv = 1.f / lt;
  if (qv && qrow >= 0) {
    bf16* op = g.out + (long long)qrow * g.C + hh * WHD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = to_bf16(o[4 * g4 + j] * inv);
      *(bf16x4*)(op + 8 * g4 + 4 * half) = v;
    }
  }
  if (qv && half == 0) g.lse2[((long long)w * g.H + hh) * g.N + q] = m + __log2f(lt);
}

// ------------------------------------------------------------------------------------- backward: dQ (+ delta, dS)
template <bool TABL>
__global__ __launch_bounds__(WL_NW * 64) void wl_dq_kernel(WinLongArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WinArgs& g = a.g;
  int w, hh, qc;
  wl_item(a, w, hh, qc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  WlLds L;
  wl_setup<TABL>(a, smem, L, w, hh);
  const int q = (qc * WL_NW + wave) * 32 + (lane & 31);
  const bool qv = q < g.N;
  const bool active = (qc * WL_NW + wave) * 32 < g.N;
  const int qrow = qv ? L.row[q] : -2;
  const int qm = qv ? L.meta[q] : 0;
  const int base = (qm & 0xffff) + a.c0, rq = (qm >> 16) & 31;
  bf16x8 qf[2], df[2];
  float dsum = 0.f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    qf[ks] = wl_load8(g, L, qrow, 0, hh, ks * 16 + 8 * half);
    df[ks] = wl_load8_out(g, g.dout, qrow, hh, ks * 16 + 8 * half);   // padded queries are cropped: dO = 0
    const bf16x8 ov = wl_load8_out(g, g.o, qrow, hh, ks * 16 + 8 * half);
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum = fmaf(to_f32(df[ks][j]), to_f32(ov[j]), dsum);
  }
  const float delta = wave_sum_xor32(dsum);
  const long long rc_off = ((long long)w * g.H + hh) * g.N + q;
  const float lse = qv ? g.lse2[rc_off] : 1.0e30f;   // beyond N: P = 0
  if (qv && half == 0) a.delta[rc_off] = delta;
  f32x16 ndl;
#pragma unroll
  for (int i = 0; i < 16; ++i) ndl[i] = -delta;
  bf16* dsrow = nullptr;
  if (a.ds && qv)   // item layout [key tile][query][32 keys]: + kt * N * 32 per tile
    dsrow = a.ds + (long long)(blockIdx.x / a.nqc) * g.N * g.Npad + (long long)q * 32 + 16 * half;
  wl_st_tile(L, 0, wl_ld_kv(g, L, hh, 0));
  __syncthreads();
  f32x16 dq = {};
  for (int kt = 0; kt < g.nkt; ++kt) {
    const bf16* Kt = L.tile + (kt & 1) * 2 * WL_TILE;
    const bf16* Vt = Kt + WL_TILE;
    bf16x8 nxt;
    if (kt + 1 < g.nkt) nxt = wl_ld_kv(g, L, hh, kt + 1);
    if (active) {
      f32x16 s = mfma32(frag_row(Kt, WLD, 0, 0, lane), qf[0], f32x16{});
      s = mfma32(frag_row(Kt, WLD, 0, 16, lane), qf[1], s);
      f32x16 dp = mfma32(frag_row(Vt, WLD, 0, 0, lane), df[0], ndl);
      dp = mfma32(frag_row(Vt, WLD, 0, 16, lane), df[1], dp);
      wl_logits<false, TABL>(a, L, hh, base, rq, kt * 32, half, s);
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = exp2_fast(s[i] - lse) * dp[i];   // dS^T (natural-log units)
      const bf16x8 lo = pack8<0>(s), hi = pack8<1>(s);
      if (a.ds) {   // (wave-uniform)
        // This lane holds keys 8 g4 + 4 half + j of its query; lanes l and l ^ 32 hold the two halves of one query.
        // One v_permlane32_swap per dword hands the lower half its partner's keys 8 g4 + 4 .. + 7 of g4 = 0, 1 and
        // the upper half its partner's keys 16 + 8 g4 .. + 3, so each lane owns 16 consecutive keys (16 half ..) and
        // the wave stores the 32 x 32 tile as 2 KB of consecutive bytes: ds[kt][q][32].
        const u32x4 lu = __builtin_bit_cast(u32x4, lo), hu = __builtin_bit_cast(u32x4, hi);
        u32x4 o[2];
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
          for (int wd = 0; wd < 2; ++wd) {
            const auto r = __builtin_amdgcn_permlane32_swap(lu[2 * g2 + wd], hu[2 * g2 + wd], false, false);
            o[g2][wd] = r[0];
            o[g2][2 + wd] = r[1];
          }
        if (dsrow) {
          bf16* d = dsrow + (long long)kt * g.N * 32;
          *(u32x4*)(d) = o[0];
          *(u32x4*)(d + 8) = o[1];
        }
      }
      dq = mfma32(frag_tr<0>(Kt, WLD, 0, 0, lane), lo, dq);
      dq = mfma32(frag_tr<1>(Kt, WLD, 0, 0, lane), hi, dq);
    }
    if (kt + 1 < g.nkt) wl_st_tile(L, (kt + 1) & 1, nxt);
    __syncthreads();
  }
  if (qv && qrow >= 0) {
    bf16* dqp = g.dqkv + (long long)qrow * 3 * g.C + hh * WHD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = to_bf16(dq[4 * g4 + j] * g.scale);
      *(bf16x4*)(dqp + 8 * g4 + 4 * half) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------ backward: dK, dV
template <bool TABL>
__global__ __launch_bounds__(WL_NW * 64) void wl_dkv_kernel(WinLongArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const WinArgs& g = a.g;
  int w, hh, kc;
  wl_item(a, w, hh, kc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  WlLds L;
  wl_setup<TABL>(a, smem, L, w, hh);
  const int key = (kc * WL_NW + wave) * 32 + (lane & 31);
  const bool kv = key < g.N;
  const bool active = (kc * WL_NW + wave) * 32 < g.N;
  const int krow = kv ? L.row[key] : -2;
  const int km = kv ? L.meta[key] : 0;
  const int base = a.c0 - (km & 0xffff), rk = (km >> 16) & 31;
  bf16x8 kf[2], vf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    kf[ks] = wl_load8(g, L, krow, 1, hh, ks * 16 + 8 * half);
    vf[ks] = wl_load8(g, L, krow, 2, hh, ks * 16 + 8 * half);
  }
  const float* lseg = g.lse2 + ((long long)w * g.H + hh) * g.N;
  const float* delg = a.delta + ((long long)w * g.H + hh) * g.N;
  // this thread's piece of query tile qt: a 16-byte chunk of Q (threads 0-127) or dO (128-255); threads 0-31 also
  // lse2 and threads 32-63 -delta of the tile's queries (1e30 / 0 beyond N: P = 0)
  auto ld_tile = [&](int qt, bf16x8& v, float& rcv) __attribute__((always_inline)) {
    const int t = threadIdx.x & 127;
    const int row = L.row[qt * 32 + (t >> 2)];
    v = threadIdx.x < 128 ? wl_load8(g, L, row, 0, hh, (t & 3) * 8) : wl_load8_out(g, g.dout, row, hh, (t & 3) * 8);
    if (threadIdx.x < 64) {
      const int n = qt * 32 + (threadIdx.x & 31);
      if (threadIdx.x < 32) rcv = n < g.N ? lseg[n] : 1.0e30f;
      else rcv = n < g.N ? -delg[n] : 0.f;
    }
  };
  auto st_tile = [&](int buf, bf16x8 v, float rcv) __attribute__((always_inline)) {
    wl_st_tile(L, buf, v);
    if (threadIdx.x < 64) L.rc[buf * 64 + threadIdx.x] = rcv;
  };
  {
    bf16x8 v;
    float rcv = 0.f;
    ld_tile(0, v, rcv);
    st_tile(0, v, rcv);
  }
  __syncthreads();
  f32x16 dk = {}, dv = {};
  for (int qt = 0; qt < g.nqb; ++qt) {
    const bf16* Qt = L.tile + (qt & 1) * 2 * WL_TILE;
    const bf16* Dt = Qt + WL_TILE;
    const float* rc = L.rc + (qt & 1) * 64;
    bf16x8 nxt;
    float nrc = 0.f;
    if (qt + 1 < g.nqb) ld_tile(qt + 1, nxt, nrc);
    if (active) {
      f32x16 dp, lz;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {   // row constants of queries qt*32 + 8 g4 + 4 half + j
        const f32x4 l4 = *(const f32x4*)(rc + 8 * g4 + 4 * half);
        const f32x4 d4 = *(const f32x4*)(rc + 32 + 8 * g4 + 4 * half);
#pragma unroll
        for (int j = 0; j < 4; ++j) { lz[4 * g4 + j] = l4[j]; dp[4 * g4 + j] = d4[j]; }
      }
      f32x16 s = mfma32(frag_row(Qt, WLD, 0, 0, lane), kf[0], f32x16{});
      s = mfma32(frag_row(Qt, WLD, 0, 16, lane), kf[1], s);
      dp = mfma32(frag_row(Dt, WLD, 0, 0, lane), vf[0], dp);
      dp = mfma32(frag_row(Dt, WLD, 0, 16, lane), vf[1], dp);
      wl_logits<true, TABL>(a, L, hh, base, rk, qt * 32, half, s);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = exp2_fast(s[i] - lz[i]);   // P (query rows, key on lane)
        dp[i] = s[i] * dp[i];             // dS
      }
      dv = mfma32(frag_tr<0>(Dt, WLD, 0, 0, lane), pack8<0>(s), dv);
      dv = mfma32(frag_tr<1>(Dt, WLD, 0, 0, lane), pack8<1>(s), dv);
      dk = mfma32(frag_tr<0>(Qt, WLD, 0, 0, lane), pack8<0>(dp), dk);
      dk = mfma32(frag_tr<1>(Qt, WLD, 0, 0, lane), pack8<1>(dp), dk);
    }
    if (qt + 1 < g.nqb) st_tile((qt + 1) & 1, nxt, nrc);
    __syncthreads();
  }
  if (kv && krow >= 0) {
    bf16* basep = g.dqkv + (long long)krow * 3 * g.C + hh * WHD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 v0, v1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v0[j] = to_bf16(dk[4 * g4 + j] * g.scale);
        v1[j] = to_bf16(dv[4 * g4 + j]);
      }
      *(bf16x4*)(basep + g.C + 8 * g4 + 4 * half) = v0;
      *(bf16x4*)(basep + 2 * g.C + 8 * g4 + 4 * half) = v1;
    }
  }
  // padded voxels: their k, v are the qkv bias. One (k | v) x 32 partial per workgroup: lanes in a fixed shuffle
  // tree, then the waves in wave order through LDS (the tiles are dead after the loop's last barrier)
  if (a.pad_part != nullptr) {
    const bool padk = kv && krow == -1;
    float* pw = (float*)L.tile + wave * 64;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float sk = padk ? dk[i] * g.scale : 0.f, sv = padk ? dv[i] : 0.f;
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) {
        sk += __shfl_xor(sk, o);
        sv += __shfl_xor(sv, o);
      }
      if ((lane & 31) == 0) {
        const int d = 8 * (i >> 2) + 4 * half + (i & 3);
        pw[d] = sk;
        pw[32 + d] = sv;
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      float acc = 0.f;
      for (int v = 0; v < WL_NW; ++v) acc += ((const float*)L.tile)[v * 64 + threadIdx.x];
      a.pad_part[(long long)blockIdx.x * 64 + threadIdx.x] = acc;
    }
  }
}

// dbias_pad[third * C + h * 32 + d]: 0 for the q third (padded queries are cropped), for k | v the sum of the
// workgroup partials of head h in a fixed order (strided per thread, then a tree). One workgroup per (head, value).
__global__ __launch_bounds__(256) void wl_pad_reduce_kernel(WinLongArgs a, float* dbias_pad) {
  __shared__ float red[256];
  const WinArgs& g = a.g;
  const int hh = blockIdx.x / 96, t = blockIdx.x % 96;
  if (t < 32) {
    if (threadIdx.x == 0) dbias_pad[hh * WHD + t] = 0.f;
    return;
  }
  const int rows = g.Bw * a.nqc;   // (window, chunk) partials of this head
  float acc = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const int w = r / a.nqc, kc = r % a.nqc;
    acc += a.pad_part[(((long long)w * g.H + hh) * a.nqc + kc) * 64 + (t - 32)];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dbias_pad[(t < 64 ? g.C : 2 * g.C) + hh * WHD + (t & 31)] = red[0];
}

// Table gradient of one chunk of items: grid (ceil(n_tab / 256), nrg, H); thread = table row r, for the raster rows
// (runs of fw_last queries along the last axis) [rg * rpr, (rg + 1) * rpr) of the full window and head blockIdx.z.
// part (nrg, n_tab, H) carries the sum from chunk to chunk: a head's first item starts it at 0, and a thread adds its
// terms in (item, row, position) order whatever the chunking, so the budget does not change a bit of the result.
// Offset d_s = r_s - (fw_s - 1) per axis: the query at coordinates c pairs with the key at c - d when that lies in the
// full window and below N, key = q - D, D = sum_s d_s * stride_s. A row whose leading coordinates have no partner is
// skipped whole (the 64 rows r of a wave share their leading offsets but for one or two steps); along the last axis
// neighbouring r read neighbouring keys of the same query row: coalesced.
__global__ __launch_bounds__(256) void wl_dtab_kernel(WinLongArgs a) {
  const WinArgs& g = a.g;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.ntab) return;
  const int rg = blockIdx.y, hh = blockIdx.z;
  const int last = g.nd - 1, fl = a.fw[last];
  int d0 = 0, d1 = 0, dl = 0, D = 0, stride = 1;   // offsets of the two leading axes (d1 unused in 2-D) and the last
  for (int s = last; s >= 0; --s) {
    const int d = (r / a.wgt[s]) % (2 * a.fw[s] - 1) - (a.fw[s] - 1);
    if (s == last) dl = d;
    else if (s == last - 1) d1 = d;
    else d0 = d;
    D += d * stride;
    stride *= a.fw[s];
  }
  if (g.nd == 2) { d0 = d1; d1 = 0; }
  const int f0 = a.fw[0], f1 = g.nd == 3 ? a.fw[1] : 1;
  const int lo = dl > 0 ? dl : 0, hi = dl < 0 ? fl + dl : fl;
  float* pp = a.part + ((long long)rg * a.ntab + r) * g.H + hh;
  float acc = a.i0 > hh ? *pp : 0.f;   // an earlier chunk held an item of this head
  const int nrows = (g.N + fl - 1) / fl;
  const int row0 = rg * a.rpr, row1 = min(nrows, row0 + a.rpr);
  const int first = a.i0 + ((hh - a.i0 % g.H) + g.H) % g.H;
  for (int item = first; item < a.i0 + a.ni; item += g.H) {
    const bf16* ds = a.ds + (long long)(item - a.i0) * g.N * g.Npad;
    for (int row = row0; row < row1; ++row) {
      const int c1 = row % f1, c0 = row / f1;   // leading coordinates of the row (c0 < f0 as row < nrows)
      if (c1 - d1 < 0 || c1 - d1 >= f1 || c0 - d0 < 0 || c0 - d0 >= f0) continue;
      const int qb = row * fl;
#pragma unroll 4
      for (int c = 0; c < fl; ++c) {   // (q = qb + c, key = q - D) at ds[key / 32][q][key % 32]
        const int q = qb + c, k = q - D;
        const bool ok = c >= lo && c < hi && q < g.N && k < g.N;
        const float v = ok ? to_f32(ds[((long long)(k >> 5) * g.N + q) * 32 + (k & 31)]) : 0.f;
        acc += v;
      }
    }
  }
  *pp = acc;
}

// rel(q, k) as the attention kernels evaluate it (tests): idx (N, N) int32
__global__ __launch_bounds__(256) void wl_index_kernel(WinLongArgs a, int* idx) {
  const long long e = blockIdx.x * 256LL + threadIdx.x;
  const int N = a.g.N;
  if (e >= (long long)N * N) return;
  const int q = (int)(e / N), k = (int)(e % N);
  idx[e] = wl_code(a, q) - wl_code(a, k) + a.c0;
}

static double wl_budget_mb() {   // read once per process, like the other hooks
  static const double v = getenv("LCI_WIN_LONG_WS_MB") ? atof(getenv("LCI_WIN_LONG_WS_MB")) : 256.0;
  return v;
}

static int wl_fill(WinLongArgs& a, const int* geo, const int* full, float scale) {
  LCI_CHECK(geo && full, "window_long: null geometry");
  LCI_CHECK(geo[0] == 1, "window_long: grid mode only (the pre-partitioned call stops at %d tokens)", WMAXN);
  if (win_fill(a.g, geo, scale, WL_MAXN)) return 1;
  const WinArgs& g = a.g;
  long long ntab = 1, nfull = 1;
  for (int s = 0; s < 3; ++s) { a.fw[s] = 1; a.wgt[s] = 0; }
  for (int s = g.nd - 1; s >= 0; --s) {
    a.fw[s] = full[s];
    LCI_CHECK(a.fw[s] >= g.ws[s] && a.fw[s] <= WL_MAXN, "window_long: full window %d < window %d on axis %d",
              a.fw[s], g.ws[s], s);
    a.wgt[s] = (int)ntab;
    ntab *= 2 * a.fw[s] - 1;
    nfull *= a.fw[s];
    LCI_CHECK(ntab <= WL_MAXTAB, "window_long: relative-position table of more than %d rows", WL_MAXTAB);
  }
  LCI_CHECK(g.N <= nfull, "window_long: N %d exceeds the full window", g.N);
  a.ntab = (int)ntab;
  a.c0 = (a.ntab - 1) / 2;
  a.nqc = (g.N + 32 * WL_NW - 1) / (32 * WL_NW);
  a.i0 = 0;
  a.ni = g.Bw * g.H;
  const int nrows = (g.N + a.fw[g.nd - 1] - 1) / a.fw[g.nd - 1];
  a.rpr = (nrows + 31) / 32;
  a.nrg = (nrows + a.rpr - 1) / a.rpr;
  LCI_CHECK((long long)g.Bw * g.H * a.nqc < (1LL << 31), "window_long: too many workgroups");
  return 0;
}

static size_t wl_part_bytes(const WinLongArgs& a) {
  return ((size_t)a.nrg * a.ntab * a.g.H * 4 + 255) / 256 * 256;
}
// (window, head) items whose dS one pass holds within the budget (at least one)
static long long wl_items_per_pass(const WinLongArgs& a) {
  const double item = (double)a.g.N * a.g.Npad * 2;
  const double room = wl_budget_mb() * 1048576.0 - (double)wl_part_bytes(a);
  long long n = room > item ? (long long)(room / item) : 1;
  return std::max<long long>(1, std::min<long long>(n, (long long)a.g.Bw * a.g.H));
}

template <bool TABL>
static int wl_launch_fwd(const WinLongArgs& a, hipStream_t s) {
  const size_t lds = wl_lds_bytes(a, TABL);
  (void)hipFuncSetAttribute((const void*)wl_fwd_kernel<TABL>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(wl_fwd_kernel<TABL>, dim3(a.ni * a.nqc), dim3(WL_NW * 64), lds, s, a);
  LCI_LAUNCH_CHECK();
  return 0;
}
template <bool TABL>
static int wl_launch_dq(const WinLongArgs& a, hipStream_t s) {
  const size_t lds = wl_lds_bytes(a, TABL);
  (void)hipFuncSetAttribute((const void*)wl_dq_kernel<TABL>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(wl_dq_kernel<TABL>, dim3(a.ni * a.nqc), dim3(WL_NW * 64), lds, s, a);
  LCI_LAUNCH_CHECK();
  return 0;
}
template <bool TABL>
static int wl_launch_dkv(const WinLongArgs& a, hipStream_t s) {
  const size_t lds = wl_lds_bytes(a, TABL);
  (void)hipFuncSetAttribute((const void*)wl_dkv_kernel<TABL>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(wl_dkv_kernel<TABL>, dim3(a.ni * a.nqc), dim3(WL_NW * 64), lds, s, a);
  LCI_LAUNCH_CHECK();
  return 0;
}

}  // namespace lci

using namespace lci;

extern "C" int lci_window_long_fwd(const void* qkv, const float* qkv_bias, const float* table, void* out, float* lse2,
                                   const int* geo, const int* full, float scale, void* stream) {
  WinLongArgs a{};
  if (wl_fill(a, geo, full, scale)) return 1;
  LCI_CHECK(qkv && table && out && lse2, "window_long_fwd: null argument");
  LCI_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 7) == 0, "window_long_fwd: qkv / out alignment");
  a.g.qkv = (const bf16*)qkv; a.g.qkv_bias = qkv_bias; a.table = table; a.g.out = (bf16*)out; a.g.lse2 = lse2;
  return a.ntab <= WL_TAB_LDS ? wl_launch_fwd<true>(a, (hipStream_t)stream)
                              : wl_launch_fwd<false>(a, (hipStream_t)stream);
}

extern "C" long long lci_window_long_pad_ws_elems(const int* geo, const int* full) {
  WinLongArgs a{};
  if (wl_fill(a, geo, full, 1.f)) return -1;
  return (long long)a.g.Bw * a.g.H * a.nqc * 64;
}

extern "C" long long lci_window_long_ws_bytes(const int* geo, const int* full) {
  WinLongArgs a{};
  if (wl_fill(a, geo, full, 1.f)) return -1;
  return (long long)wl_part_bytes(a) + wl_items_per_pass(a) * a.g.N * a.g.Npad * 2;
}

extern "C" long long lci_window_long_ws_items(const int* geo, const int* full) {
  WinLongArgs a{};
  if (wl_fill(a, geo, full, 1.f)) return -1;
  return wl_items_per_pass(a);
}

extern "C" int lci_window_long_bwd(const void* qkv, const float* qkv_bias, const float* table, const void* out,
                                   const void* dout, const float* lse2, void* dqkv, float* delta, float* dbias_pad,
                                   float* pad_ws, float* dtable, void* ws, const int* geo, const int* full,
                                   float scale, void* stream) {
  WinLongArgs a{};
  if (wl_fill(a, geo, full, scale)) return 1;
  LCI_CHECK(qkv && table && out && dout && lse2 && dqkv && delta, "window_long_bwd: null argument");
  LCI_CHECK(!dbias_pad || pad_ws, "window_long_bwd: dbias_pad needs the pad_ws workspace");
  LCI_CHECK(!dtable || ws, "window_long_bwd: dtable needs the workspace");
  LCI_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)dout & 15) == 0 &&
                ((uintptr_t)dqkv & 7) == 0 && ((uintptr_t)ws & 255) == 0,
            "window_long_bwd: qkv / out / dout / dqkv / ws alignment");
  hipStream_t s = (hipStream_t)stream;
  a.g.qkv = (const bf16*)qkv; a.g.qkv_bias = qkv_bias; a.table = table; a.g.o = (const bf16*)out;
  a.g.dout = (const bf16*)dout; a.g.lse2 = (float*)lse2; a.g.dqkv = (bf16*)dqkv; a.delta = delta;
  const bool tabl = a.ntab <= WL_TAB_LDS;
  const int items = a.g.Bw * a.g.H;
  if (dtable) {
    a.part = (float*)ws;
    a.ds = (bf16*)((char*)ws + wl_part_bytes(a));
    const int per = (int)wl_items_per_pass(a);
    for (int i0 = 0; i0 < items; i0 += per) {
      a.i0 = i0;
      a.ni = std::min(per, items - i0);
      if (tabl ? wl_launch_dq<true>(a, s) : wl_launch_dq<false>(a, s)) return 3;
      hipLaunchKernelGGL(wl_dtab_kernel, dim3((a.ntab + 255) / 256, a.nrg, a.g.H), dim3(256), 0, s, a);
      LCI_LAUNCH_CHECK();
    }
    if (ordered_sum(a.part, (long long)a.ntab * a.g.H, 1, a.nrg, (long long)a.ntab * a.g.H, dtable, s)) return 1;
    a.ds = nullptr;
  } else {
    if (tabl ? wl_launch_dq<true>(a, s) : wl_launch_dq<false>(a, s)) return 3;
  }
  a.i0 = 0;
  a.ni = items;
  a.pad_part = dbias_pad ? pad_ws : nullptr;
  if (tabl ? wl_launch_dkv<true>(a, s) : wl_launch_dkv<false>(a, s)) return 3;
  if (dbias_pad) {
    hipLaunchKernelGGL(wl_pad_reduce_kernel, dim3(a.g.H * 96), dim3(256), 0, s, a, dbias_pad);
    LCI_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int lci_window_long_index(const int* geo, const int* full, int* idx, void* stream) {
  WinLongArgs a{};
  if (wl_fill(a, geo, full, 1.f)) return 1;
  LCI_CHECK(idx, "window_long_index: null output");
  const long long n = (long long)a.g.N * a.g.N;
  hipLaunchKernelGGL(wl_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, idx);
  LCI_LAUNCH_CHECK();
  return 0;
}
