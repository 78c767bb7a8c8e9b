// Task metrics of the reference's step tail (metrics/metrics_base.py:150-180, metrics/metrics_utils.py:10-28):
// SSIM and PSNR for task_type=enhance, samplewise macro F1 for task_type=seg, each as one fused op that leaves its
// result in device memory (the reference runs torchmetrics and pulls every value to the host with .item()).
//
// lci_enhance_metrics, outputs p and targets t of shape (B, C, T, H, W):
//   em_stats           streaming pass: per workgroup min p, max p, min t, max t and sum (p - t)^2.
//   em_stats_finalize  one workgroup: R = max(max p - min p, max t - min t), c1 = (0.01 R)^2, c2 = (0.03 R)^2 and
//                      psnr = 10 log10(R'^2 / (SSE / N)) with the zero-anchored R' = max(max t, 0) - min(min t, 0),
//                      left in device memory for the next kernel.
//   em_ssim            the 11-tap gaussian window (sigma 1.5) over the windowed axes, for interior voxels only (the
//                      kept values of torchmetrics' pad-convolve-crop never see the padding). One workgroup owns a
//                      TH x TW patch of interior voxels of one (b, c) and, in 3-D, a run of TC interior planes. Per
//                      input plane: p and t with the 10-voxel apron in LDS, the W sweep of the five moments
//                      (p, t, p^2, t^2, pt formed on the fly), the H sweep, and in 3-D a T sweep held in registers
//                      as a sliding bank of 11 partial sums per moment (A[k] <- g[10 - k] v + A[k + 1]), so a plane
//                      is read once however many output planes it feeds. Writes the patch's sum of s.
//   em_ssim_finalize   the per-workgroup sums added in f64 in a fixed order, divided by the number of interior voxels.
// lci_seg_f1, logits (B, C, S) and labels (B, S):
//   f1_count           first-maximum argmax over C per position, tp / fp / fn per class counted in per-wave LDS
//                      counters (integer atomics), one partial per workgroup.
//   f1_finalize        per sample: the partials added up (integer LDS atomics: exact in any order) -> counts
//                      (B, C, 3), and the sample's F1 in f64.
//   f1_mean            the mean over the samples.
// No float atomics and no host sync: results are bitwise reproducible. A NaN input propagates to ssim and psnr.
#include "common.hpp"

#include <math.h>

namespace lci {

constexpr int EM_THREADS = 256;
constexpr int EM_CHUNK = 4096;                                   // stats pass: elements per workgroup
constexpr int EM_NSTAT = 5;                                      // min p, max p, min t, max t, sse
constexpr int EM_R = 5, EM_K = 11;                               // window half-width and taps
constexpr int EM_TC = 6, EM_TH = 16, EM_TW = 32;                 // interior planes / rows / columns per workgroup
constexpr int EM_EH = EM_TH + 2 * EM_R, EM_EW = EM_TW + 2 * EM_R;
constexpr int EM_VPT = EM_TH * EM_TW / EM_THREADS;               // voxels of a plane per thread
constexpr int EM_NF = 5;                                         // moments: p, t, p^2, t^2, pt

struct EmWindow {
  float g[EM_K];
};

template <typename T> __device__ __forceinline__ float em_ld(const T* p, long long i) { return (float)p[i]; }

// Fixed-order reductions over the 256 threads (xor butterflies in a wave, then the four waves in order).
template <typename Op>
__device__ __forceinline__ float em_block_reduce(float v, float* red, Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(red[0], red[1]), op(red[2], red[3]));
}

struct EmMin { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
struct EmMax { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct EmAdd { __device__ float operator()(float a, float b) const { return a + b; } };

template <typename TP, typename TG>
__global__ __launch_bounds__(EM_THREADS) void em_stats(const TP* __restrict__ p, const TG* __restrict__ t,
                                                       float* __restrict__ part, long long n) {
  __shared__ float red[4];
  const long long e0 = (long long)blockIdx.x * EM_CHUNK + threadIdx.x;
  float lo_p = INFINITY, hi_p = -INFINITY, lo_t = INFINITY, hi_t = -INFINITY, sse = 0.f;
#pragma unroll 4
  for (int q = 0; q < EM_CHUNK / EM_THREADS; ++q) {
    const long long i = e0 + (long long)EM_THREADS * q;
    if (i < n) {
      const float a = em_ld(p, i), b = em_ld(t, i), d = a - b;
      lo_p = fminf(lo_p, a); hi_p = fmaxf(hi_p, a);
      lo_t = fminf(lo_t, b); hi_t = fmaxf(hi_t, b);
      sse = fmaf(d, d, sse);
    }
  }
  const float r0 = em_block_reduce(lo_p, red, EmMin()), r1 = em_block_reduce(hi_p, red, EmMax());
  const float r2 = em_block_reduce(lo_t, red, EmMin()), r3 = em_block_reduce(hi_t, red, EmMax());
  const float r4 = em_block_reduce(sse, red, EmAdd());
  if (threadIdx.x == 0) {
    float* o = part + (long long)blockIdx.x * EM_NSTAT;
    o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4;
  }
}

// stats[4] = {c1, c2, R, psnr}; result[1] = psnr. fminf / fmaxf drop a NaN, the f64 sum of squares keeps it: a NaN
// anywhere makes R (hence ssim) and psnr NaN.
__global__ __launch_bounds__(EM_THREADS) void em_stats_finalize(const float* __restrict__ part, long long nblk,
                                                                double n, float* __restrict__ stats,
                                                                float* __restrict__ result) {
  __shared__ float mm[4][EM_THREADS];
  __shared__ double ss[EM_THREADS];
  float lo_p = INFINITY, hi_p = -INFINITY, lo_t = INFINITY, hi_t = -INFINITY;
  double sse = 0.0;
  for (long long b = threadIdx.x; b < nblk; b += EM_THREADS) {
    const float* q = part + b * EM_NSTAT;
    lo_p = fminf(lo_p, q[0]); hi_p = fmaxf(hi_p, q[1]);
    lo_t = fminf(lo_t, q[2]); hi_t = fmaxf(hi_t, q[3]);
    sse += (double)q[4];
  }
  mm[0][threadIdx.x] = lo_p; mm[1][threadIdx.x] = hi_p; mm[2][threadIdx.x] = lo_t; mm[3][threadIdx.x] = hi_t;
  ss[threadIdx.x] = sse;
  __syncthreads();
  for (int o = EM_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const int i = threadIdx.x;
      mm[0][i] = fminf(mm[0][i], mm[0][i + o]); mm[1][i] = fmaxf(mm[1][i], mm[1][i + o]);
      mm[2][i] = fminf(mm[2][i], mm[2][i + o]); mm[3][i] = fmaxf(mm[3][i], mm[3][i + o]);
      ss[i] += ss[i + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double s = ss[0];
    float R = fmaxf(mm[1][0] - mm[0][0], mm[3][0] - mm[2][0]);
    double Rp = (double)fmaxf(mm[3][0], 0.f) - (double)fminf(mm[2][0], 0.f);
    if (s != s) { R = NAN; Rp = NAN; }
    const float k1 = 0.01f * R, k2 = 0.03f * R;
    const float psnr = (float)(10.0 * log10(Rp * Rp / (s / n)));
    stats[0] = k1 * k1; stats[1] = k2 * k2; stats[2] = R; stats[3] = psnr;
    result[1] = psnr;
  }
}

__device__ __forceinline__ float em_ssim_of(const float (&v)[EM_NF], float c1, float c2) {
  const float mp = v[0], mt = v[1];
  const float vp = fmaxf(fmaf(-mp, mp, v[2]), 0.f), vt = fmaxf(fmaf(-mt, mt, v[3]), 0.f);
  const float cov = fmaf(-mp, mt, v[4]);
  const float num = (2.f * mp * mt + c1) * (2.f * cov + c2);
  const float den = (mp * mp + mt * mt + c1) * (vp + vt + c2);
  return num / den;
}

// Grid: (b c) x T chunks x H patches x W patches. Interior voxel (ot, oh, ow) is raw voxel (ot + 5, oh + 5, ow + 5) and
// its window covers raw [ot, ot + 10] x [oh, oh + 10] x [ow, ow + 10]: the apron only ever extends upwards, and a raw
// index past the sample's extent (zero-filled in LDS) feeds only interior indices past IH / IW, which are masked.
template <typename TP, typename TG, bool D3>
__global__ __launch_bounds__(EM_THREADS) void em_ssim(const TP* __restrict__ p, const TG* __restrict__ t,
                                                      const float* __restrict__ stats, float* __restrict__ part,
                                                      EmWindow win, int T, int H, int W, int nc, int nh, int nw) {
  __shared__ float sp[EM_EH * EM_EW], st[EM_EH * EM_EW];
  __shared__ float t1[EM_NF][EM_EH * EM_TW];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  unsigned blk = blockIdx.x;
  const int ow0 = (int)(blk % nw) * EM_TW; blk /= nw;
  const int oh0 = (int)(blk % nh) * EM_TH; blk /= nh;
  const int ot0 = (int)(blk % nc) * EM_TC; blk /= nc;
  const long long base = (long long)blk * T * H * W;
  const int IT = D3 ? T - 2 * EM_R : 1, IH = H - 2 * EM_R, IW = W - 2 * EM_R;
  const int nout = min(EM_TC, IT - ot0);                       // interior planes of this workgroup
  const int nin = D3 ? nout + 2 * EM_R : 1;                    // raw planes it reads, from raw plane ot0
  const float c1 = stats[0], c2 = stats[1];
  float g[EM_K];
#pragma unroll
  for (int m = 0; m < EM_K; ++m) g[m] = win.g[m];

  bool in[EM_VPT];
#pragma unroll
  for (int j = 0; j < EM_VPT; ++j) {
    const int i = tid + EM_THREADS * j;
    in[j] = oh0 + i / EM_TW < IH && ow0 + i % EM_TW < IW;
  }
  float A[EM_VPT][EM_NF][D3 ? EM_K : 1] = {};
  float acc = 0.f;
  for (int z = 0; z < nin; ++z) {
    const long long plane = base + (long long)(ot0 + z) * H * W;
    for (int i = tid; i < EM_EH * EM_EW; i += EM_THREADS) {
      const int h = oh0 + i / EM_EW, w = ow0 + i % EM_EW;
      float a = 0.f, b = 0.f;
      if (h < H && w < W) {
        const long long x = plane + (long long)h * W + w;
        a = em_ld(p, x); b = em_ld(t, x);
      }
      sp[i] = a; st[i] = b;
    }
    __syncthreads();
    for (int i = tid; i < EM_EH * EM_TW; i += EM_THREADS) {
      const int w = i % EM_TW, r = i / EM_TW;
      const float* qa = sp + r * EM_EW + w;
      const float* qb = st + r * EM_EW + w;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
      for (int m = 0; m < EM_K; ++m) {
        const float a = qa[m], b = qb[m], ga = g[m] * a, gb = g[m] * b;
        s0 += ga; s1 += gb;
        s2 = fmaf(ga, a, s2); s3 = fmaf(gb, b, s3); s4 = fmaf(ga, b, s4);
      }
      t1[0][i] = s0; t1[1][i] = s1; t1[2][i] = s2; t1[3][i] = s3; t1[4][i] = s4;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EM_VPT; ++j) {
      const int i = tid + EM_THREADS * j;                      // (h, w) of the patch = i / 32, i % 32
      float v[EM_NF];
#pragma unroll
      for (int f = 0; f < EM_NF; ++f) {
        float a = 0.f;
#pragma unroll
        for (int m = 0; m < EM_K; ++m) a = fmaf(g[m], t1[f][i + m * EM_TW], a);
        v[f] = a;
      }
      if (D3) {
#pragma unroll
        for (int f = 0; f < EM_NF; ++f) {
#pragma unroll
          for (int k = 0; k < EM_K - 1; ++k) A[j][f][k] = fmaf(g[EM_K - 1 - k], v[f], A[j][f][k + 1]);
          A[j][f][EM_K - 1] = g[0] * v[f];
        }
        if (z >= 2 * EM_R && in[j]) {                          // interior plane ot0 + z - 10 is complete
          float u[EM_NF];
#pragma unroll
          for (int f = 0; f < EM_NF; ++f) u[f] = A[j][f][0];
          acc += em_ssim_of(u, c1, c2);
        }
      } else if (in[j]) {
        acc += em_ssim_of(v, c1, c2);
      }
    }
    // the next plane's loads overwrite sp / st only after every thread passed the barrier above (W sweep done), and
    // its W sweep overwrites t1 only after the barrier that follows those loads (this H sweep done)
  }
  const float r = em_block_reduce(acc, red, EmAdd());
  if (tid == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(EM_THREADS) void em_ssim_finalize(const float* __restrict__ part, long long nblk,
                                                               double count, float* __restrict__ result) {
  __shared__ double red[EM_THREADS];
  double s = 0.0;
  for (long long b = threadIdx.x; b < nblk; b += EM_THREADS) s += (double)part[b];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = EM_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) result[0] = (float)(red[0] / count);
}

struct EmGeo {
  long long n, nstat, nssim;
  int nc, nh, nw;
  bool d3;
};

static EmGeo em_geo(long long B, long long C, long long T, long long H, long long W) {
  EmGeo g;
  g.d3 = T != 1;
  g.n = B * C * T * H * W;
  g.nstat = (g.n + EM_CHUNK - 1) / EM_CHUNK;
  g.nc = g.d3 ? (int)((T - 2 * EM_R + EM_TC - 1) / EM_TC) : 1;
  g.nh = (int)((H - 2 * EM_R + EM_TH - 1) / EM_TH);
  g.nw = (int)((W - 2 * EM_R + EM_TW - 1) / EM_TW);
  g.nssim = B * C * g.nc * g.nh * g.nw;
  return g;
}

static bool em_shape_ok(int B, int C, int T, int H, int W) {
  return B >= 1 && C >= 1 && T >= 1 && H >= EM_K && W >= EM_K && (T == 1 || T >= EM_K);
}

static long long em_align16(long long b) { return (b + 15) / 16 * 16; }

template <typename TP, typename TG>
static int em_launch(const void* p, const void* t, float* result, void* ws, int B, int C, int T, int H, int W,
                     hipStream_t st) {
  const EmGeo g = em_geo(B, C, T, H, W);
  float* stats = (float*)ws;
  float* spart = (float*)((char*)ws + 16);
  float* mpart = (float*)((char*)ws + 16 + em_align16(g.nstat * EM_NSTAT * 4));
  EmWindow win;
  double sum = 0.0, e[EM_K];
  for (int j = 0; j < EM_K; ++j) {
    const double d = (j - EM_R) / 1.5;
    e[j] = exp(-d * d / 2.0);
    sum += e[j];
  }
  for (int j = 0; j < EM_K; ++j) win.g[j] = (float)(e[j] / sum);
  hipLaunchKernelGGL((em_stats<TP, TG>), dim3((unsigned)g.nstat), dim3(EM_THREADS), 0, st, (const TP*)p,
                     (const TG*)t, spart, g.n);
  LCI_LAUNCH_CHECK();
  hipLaunchKernelGGL(em_stats_finalize, dim3(1), dim3(EM_THREADS), 0, st, (const float*)spart, g.nstat,
                     (double)g.n, stats, result);
  LCI_LAUNCH_CHECK();
  if (g.d3)
    hipLaunchKernelGGL((em_ssim<TP, TG, true>), dim3((unsigned)g.nssim), dim3(EM_THREADS), 0, st, (const TP*)p,
                       (const TG*)t, (const float*)stats, mpart, win, T, H, W, g.nc, g.nh, g.nw);
  else
    hipLaunchKernelGGL((em_ssim<TP, TG, false>), dim3((unsigned)g.nssim), dim3(EM_THREADS), 0, st, (const TP*)p,
                       (const TG*)t, (const float*)stats, mpart, win, T, H, W, g.nc, g.nh, g.nw);
  LCI_LAUNCH_CHECK();
  const double count = (double)B * C * (g.d3 ? T - 2 * EM_R : 1) * (H - 2 * EM_R) * (double)(W - 2 * EM_R);
  hipLaunchKernelGGL(em_ssim_finalize, dim3(1), dim3(EM_THREADS), 0, st, (const float*)mpart, g.nssim, count,
                     result);
  LCI_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ segmentation F1
constexpr int F1_THREADS = 256;
constexpr int F1_CHUNK = 4096;                                   // positions per workgroup and grid-stride step
constexpr int F1_MAXC = 64;
constexpr int F1_MAXWG = 1024;                                   // workgroups (partials) per sample

static int f1_wgs(long long S) {
  const long long c = (S + F1_CHUNK - 1) / F1_CHUNK;
  return (int)(c < F1_MAXWG ? c : F1_MAXWG);
}

// Grid: (b, g). part (B, G, 3 C) u32 = tp | fp | fn per class; a workgroup sees at most S < 2^31 positions.
template <typename TL>
__global__ __launch_bounds__(F1_THREADS) void f1_count(const TL* __restrict__ logits,
                                                       const long long* __restrict__ labels,
                                                       unsigned* __restrict__ part, int C, long long S, int G) {
  __shared__ unsigned cnt[F1_THREADS / 64][3 * F1_MAXC];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = blockIdx.x / G, gi = blockIdx.x % G;
  for (int i = tid; i < (F1_THREADS / 64) * 3 * F1_MAXC; i += F1_THREADS) (&cnt[0][0])[i] = 0u;
  __syncthreads();
  const TL* lg = logits + (long long)b * C * S;
  const long long* lb = labels + (long long)b * S;
  unsigned* mine = cnt[wave];
  auto tally = [&](int pred, long long l) {
    if (l == pred) {
      atomicAdd(&mine[pred], 1u);
    } else {
      atomicAdd(&mine[C + pred], 1u);
      if (l >= 0 && l < C) atomicAdd(&mine[2 * C + (int)l], 1u);
    }
  };
  // four consecutive positions per thread and load when every channel row and the labels are 16-byte aligned
  typedef TL tl4 __attribute__((ext_vector_type(4)));
  typedef long long ll2 __attribute__((ext_vector_type(2)));
  const bool vec = (S & 3) == 0 && (((uintptr_t)lg | (uintptr_t)lb) & 15) == 0 && ((S * sizeof(TL)) & 15) == 0;
  for (long long s0 = (long long)gi * F1_CHUNK; s0 < S; s0 += (long long)G * F1_CHUNK) {
    if (vec) {
      for (int q = 0; q < F1_CHUNK / (4 * F1_THREADS); ++q) {
        const long long s = s0 + 4 * (tid + F1_THREADS * q);
        if (s >= S) break;
        const ll2 l01 = *(const ll2*)(lb + s), l23 = *(const ll2*)(lb + s + 2);
        const tl4 v0 = *(const tl4*)(lg + s);
        float best[4] = {(float)v0[0], (float)v0[1], (float)v0[2], (float)v0[3]};
        int pred[4] = {0, 0, 0, 0};
#pragma unroll 4
        for (int c = 1; c < C; ++c) {
          const tl4 v = *(const tl4*)(lg + (long long)c * S + s);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float x = (float)v[k];
            if (x > best[k] || (x != x && best[k] == best[k])) { best[k] = x; pred[k] = c; }
          }
        }
        tally(pred[0], l01[0]); tally(pred[1], l01[1]); tally(pred[2], l23[0]); tally(pred[3], l23[1]);
      }
    } else {
      for (int q = 0; q < F1_CHUNK / F1_THREADS; ++q) {
        const long long s = s0 + tid + F1_THREADS * q;
        if (s >= S) break;
        float best = (float)lg[s];
        int pred = 0;
        for (int c = 1; c < C; ++c) {
          const float v = (float)lg[(long long)c * S + s];
          if (v > best || (v != v && best == best)) { best = v; pred = c; }   // first maximum; a NaN is a maximum
        }
        tally(pred, lb[s]);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * C; i += F1_THREADS)
    part[(long long)blockIdx.x * 3 * C + i] = (cnt[0][i] + cnt[1][i]) + (cnt[2][i] + cnt[3][i]);
}

// Grid: b. counts (B, C, 3) i64 = tp, fp, fn; f1b[b] f64.
__global__ __launch_bounds__(F1_THREADS) void f1_finalize(const unsigned* __restrict__ part,
                                                          long long* __restrict__ counts, double* __restrict__ f1b,
                                                          int C, int G) {
  __shared__ unsigned long long tot[3 * F1_MAXC];
  const int b = blockIdx.x, n3 = 3 * C;
  for (int i = threadIdx.x; i < n3; i += F1_THREADS) tot[i] = 0ull;
  __syncthreads();
  // the sample's G x 3C partials read once, coalesced; integer adds commute, so the LDS atomics keep the sums exact
  const unsigned* mine = part + (long long)b * G * n3;
  for (int i = threadIdx.x; i < G * n3; i += F1_THREADS) {
    const unsigned v = mine[i];
    if (v) atomicAdd(&tot[i % n3], (unsigned long long)v);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n3; i += F1_THREADS) counts[((long long)b * C + i % C) * 3 + i / C] = (long long)tot[i];
  if (threadIdx.x == 0) {
    double f = 0.0;
    if (C == 2) {                                              // the reference's 'binary' task: class 1
      const double tp = (double)tot[1], d = 2.0 * tp + (double)tot[C + 1] + (double)tot[2 * C + 1];
      f = d > 0.0 ? 2.0 * tp / d : 0.0;
    } else {                                                   // macro over the classes that occur
      int k = 0;
      for (int c = 0; c < C; ++c) {
        const double tp = (double)tot[c], d = 2.0 * tp + (double)tot[C + c] + (double)tot[2 * C + c];
        if (d > 0.0) { f += 2.0 * tp / d; ++k; }
      }
      f = k > 0 ? f / k : 0.0;
    }
    f1b[b] = f;
  }
}

__global__ void f1_mean(const double* __restrict__ f1b, int B, float* __restrict__ result) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += f1b[b];
    result[0] = (float)(s / B);
  }
}

template <typename TL>
static int f1_launch(const void* logits, const long long* labels, long long* counts, float* result, void* ws, int B,
                     int C, long long S, hipStream_t st) {
  const int G = f1_wgs(S);
  double* f1b = (double*)ws;
  unsigned* part = (unsigned*)((char*)ws + em_align16((long long)B * 8));
  hipLaunchKernelGGL((f1_count<TL>), dim3((unsigned)(B * G)), dim3(F1_THREADS), 0, st, (const TL*)logits, labels,
                     part, C, S, G);
  LCI_LAUNCH_CHECK();
  hipLaunchKernelGGL(f1_finalize, dim3((unsigned)B), dim3(F1_THREADS), 0, st, (const unsigned*)part, counts, f1b, C,
                     G);
  LCI_LAUNCH_CHECK();
  hipLaunchKernelGGL(f1_mean, dim3(1), dim3(64), 0, st, (const double*)f1b, B, result);
  LCI_LAUNCH_CHECK();
  return 0;
}

}  // namespace lci

using namespace lci;

extern "C" int lci_ssim_tile(int axis) { return axis == 0 ? EM_TC : axis == 1 ? EM_TH : axis == 2 ? EM_TW : -1; }

extern "C" long long lci_enhance_metrics_ws_bytes(int B, int C, int T, int H, int W) {
  if (!em_shape_ok(B, C, T, H, W)) return -1;
  const EmGeo g = em_geo(B, C, T, H, W);
  return 16 + em_align16(g.nstat * EM_NSTAT * 4) + em_align16(g.nssim * 4);
}

extern "C" int lci_enhance_metrics(const void* outputs, int out_dtype, const void* targets, int tgt_dtype,
                                   float* result, void* ws, int B, int C, int T, int H, int W, void* stream) {
  LCI_CHECK(em_shape_ok(B, C, T, H, W),
            "enhance_metrics: bad shape (%d, %d, %d, %d, %d): every windowed extent (H, W, and T unless T == 1) must "
            "be at least 11", B, C, T, H, W);
  LCI_CHECK((out_dtype == 0 || out_dtype == 1) && (tgt_dtype == 0 || tgt_dtype == 1),
            "enhance_metrics: dtype codes %d / %d (0 = f32, 1 = bf16)", out_dtype, tgt_dtype);
  LCI_CHECK(outputs && targets && result && ws, "enhance_metrics: null pointer");
  LCI_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)result & 3) == 0,
            "enhance_metrics: ws must be 16-byte aligned, result 4-byte");
  const EmGeo g = em_geo(B, C, T, H, W);
  LCI_CHECK(g.nstat < (1LL << 31) && g.nssim < (1LL << 31), "enhance_metrics: too many voxels for one launch");
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == 0 && tgt_dtype == 0) return em_launch<float, float>(outputs, targets, result, ws, B, C, T, H, W, st);
  if (out_dtype == 0) return em_launch<float, bf16>(outputs, targets, result, ws, B, C, T, H, W, st);
  if (tgt_dtype == 0) return em_launch<bf16, float>(outputs, targets, result, ws, B, C, T, H, W, st);
  return em_launch<bf16, bf16>(outputs, targets, result, ws, B, C, T, H, W, st);
}

extern "C" long long lci_seg_f1_ws_bytes(int B, int C, long long S) {
  if (B < 1 || C < 2 || C > F1_MAXC || S < 1 || S >= (1LL << 31)) return -1;
  return em_align16((long long)B * 8) + (long long)B * f1_wgs(S) * 3 * C * 4;
}

extern "C" int lci_seg_f1(const void* logits, int dtype, const long long* labels, long long* counts, float* result,
                          void* ws, int B, int C, long long S, void* stream) {
  LCI_CHECK(B >= 1 && S >= 1 && S < (1LL << 31), "seg_f1: bad shape (%d, %d, %lld)", B, C, S);
  LCI_CHECK(C >= 2 && C <= F1_MAXC, "seg_f1: C = %d outside [2, %d]", C, F1_MAXC);
  LCI_CHECK((long long)B * f1_wgs(S) < (1LL << 31), "seg_f1: too many samples for one launch");
  LCI_CHECK(dtype == 0 || dtype == 1, "seg_f1: dtype code %d (0 = f32, 1 = bf16)", dtype);
  LCI_CHECK(logits && labels && counts && result && ws, "seg_f1: null pointer");
  LCI_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)labels & 7) == 0 &&
                ((uintptr_t)result & 3) == 0,
            "seg_f1: ws must be 16-byte aligned, counts / labels 8-byte, result 4-byte");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) return f1_launch<float>(logits, labels, counts, result, ws, B, C, S, st);
  return f1_launch<bf16>(logits, labels, counts, result, ws, B, C, S, st);
}
