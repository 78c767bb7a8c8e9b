// CombinationEnhance loss (loss/loss_base.py:28-29: Combined_Loss(["mse", "charbonnier", "gaussian3D"], [1, 1, 1]),
// loss/loss_functions/enhancement_losses.py:18-278) as one fused forward + gradient op for one-channel volumes.
//
// With d = o - t over N = B T H W voxels and g_k = corr3d(d, w_k) (zero 'same' padding per sample, k = 0..2):
//   loss = mean(d^2) + mean(sqrt(d^2 + 1e-6)) + (1/3) sum_k mean|g_k|
//   dloss/do = (2 d + d / sqrt(d^2 + 1e-6) + (1/3) sum_k corr3d^T(sign g_k)) / N,   sign(0) = 0.
// Every w_k is an outer product of three 1-D factors of half-width <= (2, 3, 3) along (T, H, W), so each stencil is
// three 1-D passes over a tile held in LDS.
//
//   loss_tile_fwd   one workgroup per TT x TH x TW tile of one sample: d with a (2, 3, 3) halo in LDS (zeros outside
//                   the sample), the three separable stencils, the tile's partial sums of d^2, sqrt(d^2 + eps) and
//                   |g_k|, and one byte per voxel holding the three 2-bit signs (0: 0, 1: +, 2: -).
//   loss_tile_bwd   the same tiles over the sign bytes with the same halo: the transposed stencils (taps read at
//                   i - m), plus the pointwise terms, written as the gradient in the outputs' dtype.
//   loss_pointwise  T, H or W of 1: every factor's centre tap is 0, so the stencil term and its gradient vanish; one
//                   streaming pass, the gaussian partial sums stored as 0.
//   loss_finalize   the per-workgroup partial sums added in f64 in a fixed order -> [loss, mse, charbonnier, gaussian3D].
// No atomics: loss and gradient are bitwise reproducible. A NaN in the inputs propagates to the loss (the reference
// checks isnan on the host; this op never syncs).
#include "common.hpp"

namespace lci {

constexpr int LS_TT = 4, LS_TH = 8, LS_TW = 32;                 // output tile
constexpr int LS_PT = 2, LS_PH = 3, LS_PW = 3;                  // halo = the largest half-widths
constexpr int LS_ET = LS_TT + 2 * LS_PT, LS_EH = LS_TH + 2 * LS_PH, LS_EW = LS_TW + 2 * LS_PW;
constexpr int LS_TILE = LS_TT * LS_TH * LS_TW;                  // 1024 voxels
constexpr int LS_THREADS = 256;
constexpr int LS_VPT = LS_TILE / LS_THREADS;                    // voxels per thread
constexpr int LS_HALO = LS_ET * LS_EH * LS_EW;
constexpr int LS_TAPS = 7;                                      // taps per 1-D factor, centred at 3
constexpr int LS_NPART = 5;                                     // d^2, charbonnier, |g_0|, |g_1|, |g_2|
constexpr int LS_PW_CHUNK = 4096;                               // pointwise: elements per workgroup
constexpr float LS_EPS2 = 1e-6f;                                // Charbonnier eps^2 (eps = 1e-3)

template <typename T> __device__ __forceinline__ float ld_f32(const T* p, long long i) { return (float)p[i]; }
template <typename T> __device__ __forceinline__ void st_f32(T* p, long long i, float v) { p[i] = (T)v; }

// Sum of v over the workgroup's 256 threads in a fixed order (xor butterflies inside a wave, then the four waves in
// order); every thread returns the total. red: 4 floats of LDS.
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

struct TileGeo {
  int b, t0, h0, w0;
};

__device__ __forceinline__ TileGeo tile_of(unsigned blk, int nt, int nh, int nw) {
  TileGeo g;
  g.w0 = (int)(blk % nw) * LS_TW; blk /= nw;
  g.h0 = (int)(blk % nh) * LS_TH; blk /= nh;
  g.t0 = (int)(blk % nt) * LS_TT; blk /= nt;
  g.b = (int)blk;
  return g;
}

// The three 1-D passes of one separable stencil over the halo tile src (ET, EH, EW): along W into t1 (ET, EH, TW),
// along H into t2 (ET, TH, TW), along T into the caller's registers (voxel tid + 256 j of the (TT, TH, TW) tile).
// f: this stencil's factors [T | H | W][7] in global memory (uniform addresses: scalar loads). DIR = +1: correlation
// sum_m f[m] x[i + m]; DIR = -1: its transpose sum_m f[m] x[i - m]. Taps past a factor's half-width are zeros in f.
template <int DIR>
__device__ __forceinline__ void sep3(const float* src, float* t1, float* t2, const float* __restrict__ f,
                                     float (&out)[LS_VPT]) {
  const int tid = threadIdx.x;
  float ft[LS_TAPS], fh[LS_TAPS], fw[LS_TAPS];
#pragma unroll
  for (int m = 0; m < LS_TAPS; ++m) { ft[m] = f[m]; fh[m] = f[LS_TAPS + m]; fw[m] = f[2 * LS_TAPS + m]; }
  for (int i = tid; i < LS_ET * LS_EH * LS_TW; i += LS_THREADS) {
    const int w = i % LS_TW, r = i / LS_TW;
    const float* p = src + r * LS_EW + w + LS_PW;
    float a = 0.f;
#pragma unroll
    for (int m = -LS_PW; m <= LS_PW; ++m) a += fw[m + 3] * p[DIR * m];
    t1[i] = a;
  }
  __syncthreads();
  for (int i = tid; i < LS_ET * LS_TH * LS_TW; i += LS_THREADS) {
    const int w = i % LS_TW, h = (i / LS_TW) % LS_TH, et = i / (LS_TW * LS_TH);
    const float* p = t1 + (et * LS_EH + h + LS_PH) * LS_TW + w;
    float a = 0.f;
#pragma unroll
    for (int m = -LS_PH; m <= LS_PH; ++m) a += fh[m + 3] * p[DIR * m * LS_TW];
    t2[i] = a;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LS_VPT; ++j) {
    const int i = tid + LS_THREADS * j;                       // (t, h, w) of the tile = i / 256, (i / 32) % 8, i % 32
    const float* p = t2 + i + LS_PT * LS_TH * LS_TW;
    float a = 0.f;
#pragma unroll
    for (int m = -LS_PT; m <= LS_PT; ++m) a += ft[m + 3] * p[DIR * m * LS_TH * LS_TW];
    out[j] = a;
  }
  __syncthreads();   // src / t1 / t2 free for the next stencil
}

template <typename TO, typename TG>
__global__ __launch_bounds__(LS_THREADS) void loss_tile_fwd(const TO* __restrict__ o, const TG* __restrict__ tg,
                                                            const float* __restrict__ taps, uint8_t* __restrict__ smap,
                                                            float* __restrict__ part, int T, int H, int W, int nt,
                                                            int nh, int nw) {
  __shared__ float src[LS_HALO];
  __shared__ float t1[LS_ET * LS_EH * LS_TW];
  __shared__ float t2[LS_ET * LS_TH * LS_TW];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const TileGeo g = tile_of(blockIdx.x, nt, nh, nw);
  const long long base = (long long)g.b * T * H * W;
  for (int i = tid; i < LS_HALO; i += LS_THREADS) {
    const int ew = i % LS_EW, eh = (i / LS_EW) % LS_EH, et = i / (LS_EW * LS_EH);
    const int t = g.t0 - LS_PT + et, h = g.h0 - LS_PH + eh, w = g.w0 - LS_PW + ew;
    float d = 0.f;
    if (t >= 0 && t < T && h >= 0 && h < H && w >= 0 && w < W) {
      const long long x = base + ((long long)t * H + h) * W + w;
      d = ld_f32(o, x) - ld_f32(tg, x);
    }
    src[i] = d;
  }
  __syncthreads();
  bool in[LS_VPT];
  float s_sq = 0.f, s_ch = 0.f;
#pragma unroll
  for (int j = 0; j < LS_VPT; ++j) {
    const int i = tid + LS_THREADS * j;
    const int w = i % LS_TW, h = (i / LS_TW) % LS_TH, t = i / (LS_TW * LS_TH);
    in[j] = g.t0 + t < T && g.h0 + h < H && g.w0 + w < W;
    if (in[j]) {
      const float d = src[((t + LS_PT) * LS_EH + h + LS_PH) * LS_EW + w + LS_PW];
      s_sq += d * d;
      s_ch += sqrtf(d * d + LS_EPS2);
    }
  }
  unsigned bits[LS_VPT] = {};
  float s_g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float gk[LS_VPT];
    sep3<1>(src, t1, t2, taps + k * 3 * LS_TAPS, gk);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LS_VPT; ++j)
      if (in[j]) {
        s += fabsf(gk[j]);
        bits[j] |= (gk[j] > 0.f ? 1u : gk[j] < 0.f ? 2u : 0u) << (2 * k);
      }
    s_g[k] = s;
  }
#pragma unroll
  for (int j = 0; j < LS_VPT; ++j)
    if (in[j]) {
      const int i = tid + LS_THREADS * j;
      const int w = i % LS_TW, h = (i / LS_TW) % LS_TH, t = i / (LS_TW * LS_TH);
      smap[base + ((long long)(g.t0 + t) * H + g.h0 + h) * W + g.w0 + w] = (uint8_t)bits[j];
    }
  const float r0 = block_sum(s_sq, red), r1 = block_sum(s_ch, red);
  const float r2 = block_sum(s_g[0], red), r3 = block_sum(s_g[1], red), r4 = block_sum(s_g[2], red);
  if (tid == 0) {
    float* p = part + (long long)blockIdx.x * LS_NPART;
    p[0] = r0; p[1] = r1; p[2] = r2; p[3] = r3; p[4] = r4;
  }
}

template <typename TO, typename TG>
__global__ __launch_bounds__(LS_THREADS) void loss_tile_bwd(const TO* __restrict__ o, const TG* __restrict__ tg,
                                                            const float* __restrict__ taps,
                                                            const uint8_t* __restrict__ smap, TO* __restrict__ grad,
                                                            float nf, int T, int H, int W, int nt, int nh, int nw) {
  __shared__ float src[LS_HALO];
  __shared__ float t1[LS_ET * LS_EH * LS_TW];
  __shared__ float t2[LS_ET * LS_TH * LS_TW];
  __shared__ uint8_t sb[LS_HALO];
  const int tid = threadIdx.x;
  const TileGeo g = tile_of(blockIdx.x, nt, nh, nw);
  const long long base = (long long)g.b * T * H * W;
  for (int i = tid; i < LS_HALO; i += LS_THREADS) {
    const int ew = i % LS_EW, eh = (i / LS_EW) % LS_EH, et = i / (LS_EW * LS_EH);
    const int t = g.t0 - LS_PT + et, h = g.h0 - LS_PH + eh, w = g.w0 - LS_PW + ew;
    uint8_t b = 0;
    if (t >= 0 && t < T && h >= 0 && h < H && w >= 0 && w < W) b = smap[base + ((long long)t * H + h) * W + w];
    sb[i] = b;
  }
  __syncthreads();
  float acc[LS_VPT] = {};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int i = tid; i < LS_HALO; i += LS_THREADS) {
      const unsigned c = (sb[i] >> (2 * k)) & 3u;
      src[i] = c == 1u ? 1.f : c == 2u ? -1.f : 0.f;
    }
    __syncthreads();
    float gk[LS_VPT];
    sep3<-1>(src, t1, t2, taps + k * 3 * LS_TAPS, gk);
#pragma unroll
    for (int j = 0; j < LS_VPT; ++j) acc[j] += gk[j];
  }
#pragma unroll
  for (int j = 0; j < LS_VPT; ++j) {
    const int i = tid + LS_THREADS * j;
    const int w = g.w0 + i % LS_TW, h = g.h0 + (i / LS_TW) % LS_TH, t = g.t0 + i / (LS_TW * LS_TH);
    if (t < T && h < H && w < W) {
      const long long x = base + ((long long)t * H + h) * W + w;
      const float d = ld_f32(o, x) - ld_f32(tg, x);
      st_f32(grad, x, (2.f * d + d / sqrtf(d * d + LS_EPS2) + acc[j] * (1.f / 3.f)) / nf);
    }
  }
}

template <typename TO, typename TG>
__global__ __launch_bounds__(LS_THREADS) void loss_pointwise(const TO* __restrict__ o, const TG* __restrict__ tg,
                                                             TO* __restrict__ grad, float* __restrict__ part,
                                                             float nf, long long n) {
  __shared__ float red[4];
  const long long e0 = (long long)blockIdx.x * LS_PW_CHUNK + 4LL * threadIdx.x;   // group q: e0 + 1024 q .. + 3
  const bool vec = (((uintptr_t)o | (uintptr_t)tg | (uintptr_t)grad) & 15) == 0 &&
                   (long long)(blockIdx.x + 1) * LS_PW_CHUNK <= n;
  float s_sq = 0.f, s_ch = 0.f;
  if (vec) {
    typedef TO vo4 __attribute__((ext_vector_type(4)));
    typedef TG vg4 __attribute__((ext_vector_type(4)));
    vo4 ov[4];
    vg4 tv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ov[q] = *(const vo4*)(o + e0 + 1024 * q);
      tv[q] = *(const vg4*)(tg + e0 + 1024 * q);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      vo4 gv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = (float)ov[q][j] - (float)tv[q][j];
        const float c = sqrtf(d * d + LS_EPS2);
        s_sq += d * d;
        s_ch += c;
        gv[j] = (TO)((2.f * d + d / c) / nf);
      }
      *(vo4*)(grad + e0 + 1024 * q) = gv;
    }
  } else {
    for (int q = 0; q < 4; ++q)
      for (long long i = e0 + 1024 * q; i < e0 + 1024 * q + 4 && i < n; ++i) {
        const float d = ld_f32(o, i) - ld_f32(tg, i);
        const float c = sqrtf(d * d + LS_EPS2);
        s_sq += d * d;
        s_ch += c;
        st_f32(grad, i, (2.f * d + d / c) / nf);
      }
  }
  const float r0 = block_sum(s_sq, red), r1 = block_sum(s_ch, red);
  if (threadIdx.x == 0) {
    float* p = part + (long long)blockIdx.x * LS_NPART;
    p[0] = r0; p[1] = r1; p[2] = 0.f; p[3] = 0.f; p[4] = 0.f;
  }
}

// One workgroup: thread i adds partials i, i + 256, ... in f64, then a fixed tree over the 256 threads.
__global__ __launch_bounds__(LS_THREADS) void loss_finalize(const float* __restrict__ part, long long nblk, double n,
                                                            float* __restrict__ result) {
  __shared__ double red[LS_NPART][LS_THREADS];
  double s[LS_NPART] = {};
  for (long long b = threadIdx.x; b < nblk; b += LS_THREADS)
#pragma unroll
    for (int c = 0; c < LS_NPART; ++c) s[c] += (double)part[b * LS_NPART + c];
#pragma unroll
  for (int c = 0; c < LS_NPART; ++c) red[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int o = LS_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int c = 0; c < LS_NPART; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double mse = red[0][0] / n, ch = red[1][0] / n;
    const double ga = (red[2][0] + red[3][0] + red[4][0]) / (3.0 * n);
    result[0] = (float)(mse + ch + ga);
    result[1] = (float)mse;
    result[2] = (float)ch;
    result[3] = (float)ga;
  }
}

static long long loss_blocks(long long B, long long T, long long H, long long W) {
  if (T == 1 || H == 1 || W == 1) return (B * T * H * W + LS_PW_CHUNK - 1) / LS_PW_CHUNK;
  return B * ((T + LS_TT - 1) / LS_TT) * ((H + LS_TH - 1) / LS_TH) * ((W + LS_TW - 1) / LS_TW);
}

static long long loss_part_bytes(long long nblk) { return (nblk * LS_NPART * 4 + 15) / 16 * 16; }

template <typename TO, typename TG>
static int loss_launch(const void* o, const void* tg, const float* taps, void* grad, float* result, void* ws, int B,
                       int T, int H, int W, hipStream_t st) {
  const long long n = (long long)B * T * H * W, nblk = loss_blocks(B, T, H, W);
  float* part = (float*)ws;
  const float nf = (float)n;
  if (T == 1 || H == 1 || W == 1) {
    hipLaunchKernelGGL((loss_pointwise<TO, TG>), dim3((unsigned)nblk), dim3(LS_THREADS), 0, st, (const TO*)o,
                       (const TG*)tg, (TO*)grad, part, nf, n);
    LCI_LAUNCH_CHECK();
  } else {
    uint8_t* smap = (uint8_t*)ws + loss_part_bytes(nblk);
    const int nt = (T + LS_TT - 1) / LS_TT, nh = (H + LS_TH - 1) / LS_TH, nw = (W + LS_TW - 1) / LS_TW;
    hipLaunchKernelGGL((loss_tile_fwd<TO, TG>), dim3((unsigned)nblk), dim3(LS_THREADS), 0, st, (const TO*)o,
                       (const TG*)tg, taps, smap, part, T, H, W, nt, nh, nw);
    LCI_LAUNCH_CHECK();
    hipLaunchKernelGGL((loss_tile_bwd<TO, TG>), dim3((unsigned)nblk), dim3(LS_THREADS), 0, st, (const TO*)o,
                       (const TG*)tg, taps, (const uint8_t*)smap, (TO*)grad, nf, T, H, W, nt, nh, nw);
    LCI_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(loss_finalize, dim3(1), dim3(LS_THREADS), 0, st, (const float*)part, nblk, (double)n, result);
  LCI_LAUNCH_CHECK();
  return 0;
}

}  // namespace lci

using namespace lci;

extern "C" long long lci_enhance_loss_ws_bytes(int B, int T, int H, int W) {
  if (B < 1 || T < 1 || H < 1 || W < 1) return -1;
  const long long nblk = loss_blocks(B, T, H, W);
  const bool flat = T == 1 || H == 1 || W == 1;
  return loss_part_bytes(nblk) + (flat ? 0 : (long long)B * T * H * W);
}

extern "C" int lci_enhance_loss(const void* outputs, int out_dtype, const void* targets, int tgt_dtype,
                                const float* taps, void* grad, float* result, void* ws, int B, int T, int H, int W,
                                void* stream) {
  LCI_CHECK(B >= 1 && T >= 1 && H >= 1 && W >= 1, "enhance_loss: bad shape (%d, 1, %d, %d, %d)", B, T, H, W);
  LCI_CHECK((out_dtype == 0 || out_dtype == 1) && (tgt_dtype == 0 || tgt_dtype == 1),
            "enhance_loss: dtype codes %d / %d (0 = f32, 1 = bf16)", out_dtype, tgt_dtype);
  LCI_CHECK(outputs && targets && taps && grad && result && ws, "enhance_loss: null pointer");
  LCI_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)result & 3) == 0 && ((uintptr_t)taps & 3) == 0,
            "enhance_loss: ws must be 16-byte aligned, result / taps 4-byte");
  LCI_CHECK(loss_blocks(B, T, H, W) < (1LL << 31), "enhance_loss: too many voxels for one launch");
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == 0 && tgt_dtype == 0)
    return loss_launch<float, float>(outputs, targets, taps, grad, result, ws, B, T, H, W, st);
  if (out_dtype == 0) return loss_launch<float, bf16>(outputs, targets, taps, grad, result, ws, B, T, H, W, st);
  if (tgt_dtype == 0) return loss_launch<bf16, float>(outputs, targets, taps, grad, result, ws, B, T, H, W, st);
  return loss_launch<bf16, bf16>(outputs, targets, taps, grad, result, ws, B, T, H, W, st);
}
