// Window geometry shared by the resident window kernels (window.hip) and the streaming large-window kernels
// (window_long.hip): the argument block, the pad / roll / partition row map, the window type and the region ids of
// compute_mask, and the host-side geometry decoder. One definition, so both kernel families (and the index-map
// exports the tests read) evaluate the same arithmetic.
#pragma once
#include "common.hpp"

#include <stdlib.h>

namespace lci {

constexpr int WHD = 32;          // head dim (Swin: C / heads = 32 at every stage)
constexpr int WLD = 40;          // LDS row stride (elements, 80 B): b128 row reads conflict-free
constexpr int WMAXN = 768;       // max tokens per window of the resident kernels (LDS: two Npad x 80 B tiles)
constexpr float WLOG2E = 1.4426950408889634f;
constexpr float WNEG = -1.0e30f;

struct WinArgs {
  const bf16* qkv; const float* qkv_bias;  // bias (3C) f32 or null: value of padded tokens
  const float* rpb;                        // (H, N, N) f32 rpb_table[index] (table builder only)
  const float* mask;                       // WINDOWS mode: (nW, N, N) f32 or null (table builder only)
  const bf16* bias;                        // (T, H, Npad, Npad) log2-domain logit term [q][k], bf16
  const bf16* biasT;                       // the same, transposed [k][q] (backward phase 2)
  bf16* out; const bf16* o; const bf16* dout;
  float* lse2;                             // (Bw, H, N)
  bf16* dqkv; float* dbias_pad;            // bwd
  float* pad_ws;                           // bwd: (Bw, H, 64) per-workgroup pad-key dK | dV sums, or null
  bf16* dS;                                // (Bw, H, nqb, nkt, 64, 16) bf16 tiles or null
  float* drpb;                             // (H, N, N) f32 (reduction kernel)
  int mode, nd, S[3], ws[3], sh[3], Sp[3], nwin[3];
  int Bw, nW, N, Npad, nqb, nkt, C, H, masked, T;
  int dS_kl;                               // dS tiles in the key-on-lane layout (win_attn_bwd1_kernel)
  int bwd1_cnt;                            // win_attn_bwd1_kernel: per-tile dQ order counters instead of a barrier
  int order;                               // workgroup -> (window, head) order of the attention kernels (win_item)
  float scale, c;
};

// token row of window token n (>= 0), -1 for a padded voxel, and its region id (grid mode)
__device__ __forceinline__ int win_row(const WinArgs& a, int w, int n, int& rid) {
  rid = 0;
  if (a.mode == 0) return w * a.N + n;
  const int b = w / a.nW;
  int wi = w % a.nW;
  int widx[3], nidx[3];
  for (int s = a.nd - 1; s >= 0; --s) { widx[s] = wi % a.nwin[s]; wi /= a.nwin[s]; }
  int nn = n;
  for (int s = a.nd - 1; s >= 0; --s) { nidx[s] = nn % a.ws[s]; nn /= a.ws[s]; }
  long long row = b;
  bool pad = false;
  for (int s = 0; s < a.nd; ++s) {
    const int p = widx[s] * a.ws[s] + nidx[s];
    int r = 0;
    if (a.sh[s] > 0) r = p < a.Sp[s] - a.ws[s] ? 0 : (p < a.Sp[s] - a.sh[s] ? 1 : 2);
    rid = rid * 3 + r;
    int src = p + a.sh[s];
    if (src >= a.Sp[s]) src -= a.Sp[s];
    if (src >= a.S[s]) pad = true;
    row = row * a.S[s] + src;
  }
  return pad ? -1 : (int)row;
}

__device__ __forceinline__ const bf16* out_row_ptr(const WinArgs& a, const bf16* base, int w, int n, int row) {
  return base + (long long)(a.mode == 0 ? w * a.N + n : row) * a.C;
}

// window type (index into the bias table)
__device__ __forceinline__ int win_type(const WinArgs& a, int w) {
  if (a.mode == 0) return a.T > 1 ? w % a.nW : 0;
  if (!a.masked) return 0;
  int wi = w % a.nW, t = 0;
  for (int s = a.nd - 1; s >= 0; --s) {
    const int widx = wi % a.nwin[s];
    wi /= a.nwin[s];
    if (a.sh[s] > 0 && widx == a.nwin[s] - 1) t |= 1 << s;
  }
  return t;
}

// compute_mask's region id (backbone_swin.py:591-628) of window token n in a window of type t
__device__ __forceinline__ int win_region(const WinArgs& a, int t, int n) {
  int nidx[3] = {0, 0, 0};
  for (int s = a.nd - 1; s >= 0; --s) { nidx[s] = n % a.ws[s]; n /= a.ws[s]; }
  int rid = 0;
  for (int s = 0; s < a.nd; ++s) rid = rid * 3 + (((t >> s) & 1) ? (nidx[s] < a.ws[s] - a.sh[s] ? 1 : 2) : 0);
  return rid;
}

// maxn: the caller's ceiling on tokens per window (WMAXN for the resident kernels)
static inline int win_fill(WinArgs& a, const int* geo, float scale, int maxn = WMAXN) {
  // geo: [mode, nd, S0, S1, S2, ws0, ws1, ws2, sh0, sh1, sh2, Bw_or_B, nW, N, C, H]
  a.mode = geo[0]; a.nd = geo[1];
  for (int s = 0; s < 3; ++s) { a.S[s] = geo[2 + s]; a.ws[s] = geo[5 + s]; a.sh[s] = geo[8 + s]; }
  a.N = geo[13]; a.C = geo[14]; a.H = geo[15];
  LCI_CHECK(a.C == a.H * WHD, "window_attn: C %d != heads %d * 32", a.C, a.H);
  LCI_CHECK(a.N > 0 && a.N <= maxn, "window_attn: N %d unsupported (<= %d)", a.N, maxn);
  a.masked = 0;
  if (a.mode == 1) {
    int nW = 1, N = 1;
    for (int s = 0; s < a.nd; ++s) {
      LCI_CHECK(a.ws[s] > 0 && a.S[s] > 0 && a.sh[s] >= 0 && a.sh[s] < a.ws[s], "window_attn: bad geometry");
      a.Sp[s] = (a.S[s] + a.ws[s] - 1) / a.ws[s] * a.ws[s];
      a.nwin[s] = a.Sp[s] / a.ws[s];
      nW *= a.nwin[s]; N *= a.ws[s];
      if (a.sh[s] > 0) a.masked = 1;
    }
    LCI_CHECK(N == a.N, "window_attn: N %d != prod(window) %d", a.N, N);
    a.nW = nW; a.Bw = geo[11] * nW;
    a.T = a.masked ? (1 << a.nd) : 1;
  } else {
    a.Bw = geo[11]; a.nW = geo[12] > 0 ? geo[12] : 1;
    a.T = 1;   // lci_window_bias / _elems set T = nW when a mask is given
  }
  a.Npad = (a.N + 31) / 32 * 32;
  a.nqb = a.nkt = a.Npad / 32;
  a.scale = scale; a.c = scale * WLOG2E;
  static const int order_env = getenv("LCI_WIN_ORDER") ? atoi(getenv("LCI_WIN_ORDER")) : 1;   // A/B hook
  a.order = order_env;
  LCI_CHECK((long long)a.Bw * a.H < (1LL << 31), "window_attn: too many (window, head) workgroups");
  return 0;
}

}  // namespace lci
