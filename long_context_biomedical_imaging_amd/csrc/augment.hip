// Training augmentation of the recipes (data/data_utils.py:120-150: RandomAffine nearest / zero fill,
// RandomBrightnessContrast, GaussianBlur(kernel_size=(1, 3))) applied on the device from parameters the host drew:
// one record of AUG_FIELDS f32 per sample (include/lci.h states the layout and every formula).
//
// One call processes one (B, P, H, W) tensor, f32 or int64 (int64: the affine only), out of place.
//   aug_mean   only for samples with bc_on (a workgroup-uniform early exit): gathers the warped values w, sums
//              alpha * w in f64 and writes one partial per workgroup (at most AUG_MAX_PARTS per sample).
//   aug_apply  every workgroup re-adds its sample's partials in one fixed order (a few hundred values, from L2), then
//              gathers, applies brightness and the 3-tap blur along H (reflect) and stores.
// A thread owns VEC consecutive pixels of a row and stores them as one 16-byte vector when W is a multiple of VEC
// and the pointers are 16-byte aligned (VEC = 4 f32 / 2 int64), else VEC = 1. Source coordinates are evaluated in
// f64 from the f32 coefficients, so the nearest index is exact wherever the coordinate is no rounding tie. The
// gathers rely on L2: the recipes rotate by at most 10 degrees, so neighbouring lanes read neighbouring addresses.
// No atomics: bitwise reproducible from call to call. Every parameter comes from device memory: no host sync, and a
// captured call follows new parameters on replay.
#include "common.hpp"

#include <math.h>

namespace lci {

constexpr int AUG_THREADS = 256;
constexpr int AUG_FIELDS = 16;
constexpr int AUG_UNROLL = 4;                                    // vectors per thread of aug_apply
constexpr int AUG_MAX_PARTS = 256;                               // partial sums per sample (one per aug_mean workgroup)
constexpr int AUG_AFFINE_ON = 0, AUG_M = 1, AUG_BC_ON = 7, AUG_ALPHA = 8, AUG_BETA = 9, AUG_BLUR_ON = 10,
              AUG_TAPS = 11;

struct AugAffine {
  bool on;
  double m0, m1, m2, m3, m4, m5;                                 // m2, m5 include the centre offsets (W-1)/2, (H-1)/2
};

__device__ __forceinline__ AugAffine aug_affine(const float* __restrict__ p, int H, int W) {
  AugAffine a;
  a.on = p[AUG_AFFINE_ON] != 0.f;
  a.m0 = (double)p[AUG_M + 0];
  a.m1 = (double)p[AUG_M + 1];
  a.m2 = (double)p[AUG_M + 2] + 0.5 * (double)(W - 1);
  a.m3 = (double)p[AUG_M + 3];
  a.m4 = (double)p[AUG_M + 4];
  a.m5 = (double)p[AUG_M + 5] + 0.5 * (double)(H - 1);
  return a;
}

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) AugVec {
  T v[VEC];
};

// The warped values of pixels (row, j0 .. j0 + VEC - 1) of one plane. An index is used only after the range check
// (a NaN coordinate fails it), so no parameter value can make the gather leave the plane.
template <typename T, int VEC>
__device__ __forceinline__ void aug_row(const T* __restrict__ plane, const AugAffine& a, int H, int W, int row, int j0,
                                        T (&out)[VEC]) {
  if (!a.on) {
    const AugVec<T, VEC> r = *(const AugVec<T, VEC>*)(plane + (long long)row * W + j0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) out[k] = r.v[k];
    return;
  }
  const double yc = (double)row - 0.5 * (double)H + 0.5;
  const double bx = fma(a.m1, yc, a.m2), by = fma(a.m4, yc, a.m5);
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const double xc = (double)(j0 + k) - 0.5 * (double)W + 0.5;
    const double rx = rint(fma(a.m0, xc, bx)), ry = rint(fma(a.m3, xc, by));   // ties to even
    T v = (T)0;
    if (rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1)) v = plane[(int)ry * W + (int)rx];
    out[k] = v;
  }
}

// Sum over the workgroup in one fixed order; every thread gets the total.
__device__ __forceinline__ double aug_block_sum(double s, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// vector g of a sample -> plane, row, first column
__device__ __forceinline__ void aug_decode(unsigned g, unsigned wvecs, unsigned H, int VEC, unsigned& plane,
                                           int& row, int& j0) {
  const unsigned r = g / wvecs;
  j0 = (int)((g - r * wvecs) * VEC);
  plane = r / H;
  row = (int)(r - plane * H);
}

template <int VEC>
__global__ __launch_bounds__(AUG_THREADS) void aug_mean(const float* __restrict__ x, const float* __restrict__ params,
                                                        double* __restrict__ part, int P, int H, int W) {
  __shared__ double red[AUG_THREADS / 64];
  const int b = blockIdx.y;
  const float* p = params + (long long)b * AUG_FIELDS;
  if (p[AUG_BC_ON] == 0.f) return;                               // the whole workgroup
  const AugAffine aff = aug_affine(p, H, W);
  const float alpha = p[AUG_ALPHA];
  const unsigned n = (unsigned)P * H * W, vecs = n / VEC, wvecs = (unsigned)W / VEC;
  const long long hw = (long long)H * W;
  const float* xs = x + (long long)b * n;
  double acc = 0.0;
  for (unsigned g = blockIdx.x * AUG_THREADS + threadIdx.x; g < vecs; g += gridDim.x * AUG_THREADS) {
    unsigned plane;
    int row, j0;
    aug_decode(g, wvecs, (unsigned)H, VEC, plane, row, j0);
    float w[VEC];
    aug_row<float, VEC>(xs + plane * hw, aff, H, W, row, j0, w);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc += (double)__fmul_rn(alpha, w[k]);
  }
  const double tot = aug_block_sum(acc, red);
  if (threadIdx.x == 0) part[(long long)b * AUG_MAX_PARTS + blockIdx.x] = tot;
}

template <typename T, int VEC>
__global__ __launch_bounds__(AUG_THREADS) void aug_apply(const T* __restrict__ x, T* __restrict__ y,
                                                         const float* __restrict__ params,
                                                         const double* __restrict__ part, int nparts, int P, int H,
                                                         int W) {
  constexpr bool FLT = sizeof(T) == 4;
  __shared__ double red[AUG_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* p = params + (long long)b * AUG_FIELDS;
  const AugAffine aff = aug_affine(p, H, W);
  const unsigned n = (unsigned)P * H * W, vecs = n / VEC, wvecs = (unsigned)W / VEC;
  const long long hw = (long long)H * W;
  const T* xs = x + (long long)b * n;
  T* ys = y + (long long)b * n;
  bool bc = false, blur = false;
  float alpha = 1.f, shift = 0.f, t0 = 0.f, t1 = 1.f, t2 = 0.f;
  if (FLT) {
    bc = p[AUG_BC_ON] != 0.f;
    blur = p[AUG_BLUR_ON] != 0.f;
    if (bc) {                                                    // sample-uniform: every thread meets the barrier
      const double s = tid < nparts ? part[(long long)b * AUG_MAX_PARTS + tid] : 0.0;
      const float mean = (float)(aug_block_sum(s, red) / (double)n);
      alpha = p[AUG_ALPHA];
      shift = __fmul_rn(p[AUG_BETA], mean);
    }
    if (blur) { t0 = p[AUG_TAPS]; t1 = p[AUG_TAPS + 1]; t2 = p[AUG_TAPS + 2]; }
  }
#pragma unroll
  for (int u = 0; u < AUG_UNROLL; ++u) {
    const unsigned g = (blockIdx.x * AUG_UNROLL + u) * AUG_THREADS + tid;
    if (g >= vecs) break;
    unsigned plane;
    int row, j0;
    aug_decode(g, wvecs, (unsigned)H, VEC, plane, row, j0);
    const T* src = xs + plane * hw;
    AugVec<T, VEC> o;
    if (FLT && blur) {
      T a[VEC], c[VEC], d[VEC];
      aug_row<T, VEC>(src, aff, H, W, row == 0 ? 1 : row - 1, j0, a);
      aug_row<T, VEC>(src, aff, H, W, row, j0, c);
      aug_row<T, VEC>(src, aff, H, W, row == H - 1 ? H - 2 : row + 1, j0, d);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float fa = (float)a[k], fc = (float)c[k], fd = (float)d[k];
        if (bc) {
          fa = __fadd_rn(__fmul_rn(alpha, fa), shift);
          fc = __fadd_rn(__fmul_rn(alpha, fc), shift);
          fd = __fadd_rn(__fmul_rn(alpha, fd), shift);
        }
        o.v[k] = (T)fmaf(t2, fd, fmaf(t1, fc, __fmul_rn(t0, fa)));
      }
    } else {
      aug_row<T, VEC>(src, aff, H, W, row, j0, o.v);
      if (FLT && bc) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = (T)__fadd_rn(__fmul_rn(alpha, (float)o.v[k]), shift);
      }
    }
    *(AugVec<T, VEC>*)(ys + plane * hw + (long long)row * W + j0) = o;
  }
}

static int aug_parts(long long vecs) {
  const long long per = (long long)AUG_THREADS * AUG_UNROLL;
  const long long g = (vecs + per - 1) / per;
  return (int)(g > AUG_MAX_PARTS ? AUG_MAX_PARTS : g);
}

template <typename T, int VEC>
static int aug_launch(const void* x, void* y, const float* params, double* part, int B, int P, int H, int W,
                      hipStream_t st) {
  const long long vecs = (long long)P * H * W / VEC;
  const int nparts = aug_parts(vecs);
  if (sizeof(T) == 4) {
    hipLaunchKernelGGL((aug_mean<VEC>), dim3((unsigned)nparts, (unsigned)B), dim3(AUG_THREADS), 0, st,
                       (const float*)x, params, part, P, H, W);
    LCI_LAUNCH_CHECK();
  }
  const long long per = (long long)AUG_THREADS * AUG_UNROLL;
  hipLaunchKernelGGL((aug_apply<T, VEC>), dim3((unsigned)((vecs + per - 1) / per), (unsigned)B), dim3(AUG_THREADS), 0,
                     st, (const T*)x, (T*)y, params, (const double*)part, nparts, P, H, W);
  LCI_LAUNCH_CHECK();
  return 0;
}

}  // namespace lci

using namespace lci;

extern "C" long long lci_augment_ws_bytes(int B, int P, int H, int W) {
  if (B < 1 || B > 65535 || P < 1 || H < 1 || W < 1 || (long long)P * H * W >= (1LL << 31)) return -1;
  return (long long)B * AUG_MAX_PARTS * 8;
}

extern "C" int lci_augment(const void* x, void* y, int dtype, const float* params, void* ws, int B, int P, int H,
                           int W, void* stream) {
  LCI_CHECK(dtype == 0 || dtype == 2, "augment: dtype code %d (0 = f32, 2 = int64)", dtype);
  LCI_CHECK(B >= 1 && B <= 65535 && P >= 1 && H >= 1 && W >= 1, "augment: B = %d (1 .. 65535), P = %d, H = %d, W = %d",
            B, P, H, W);
  const long long n = (long long)P * H * W;
  LCI_CHECK(n < (1LL << 31), "augment: %lld elements per sample (below 2^31)", n);
  LCI_CHECK(dtype != 0 || H >= 2, "augment: H = %d; the reflect-padded blur along H needs H >= 2", H);
  LCI_CHECK(x && y && params && ws, "augment: null pointer");
  const uintptr_t es = dtype == 0 ? 4 : 8, xa = (uintptr_t)x, ya = (uintptr_t)y;
  LCI_CHECK(xa % es == 0 && ya % es == 0 && ((uintptr_t)params & 3) == 0 && ((uintptr_t)ws & 15) == 0,
            "augment: x / y must be aligned to their element, params to 4 bytes, ws to 16");
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)n * es;
  LCI_CHECK(xa + bytes <= ya || ya + bytes <= xa, "augment: x and y overlap (the op is out of place)");
  hipStream_t st = (hipStream_t)stream;
  const bool al16 = ((xa | ya) & 15) == 0;
  if (dtype == 0)
    return al16 && W % 4 == 0 ? aug_launch<float, 4>(x, y, params, (double*)ws, B, P, H, W, st)
                              : aug_launch<float, 1>(x, y, params, (double*)ws, B, P, H, W, st);
  return al16 && W % 2 == 0 ? aug_launch<long long, 2>(x, y, params, (double*)ws, B, P, H, W, st)
                            : aug_launch<long long, 1>(x, y, params, (double*)ws, B, P, H, W, st);
}
