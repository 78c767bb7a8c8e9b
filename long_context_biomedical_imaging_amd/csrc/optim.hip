// Adam / AdamW parameter update over a list of f32 tensors, one launch per up to ADAM_MAXT tensors.
//
// The trainer's optimizer step (trainer_base.py:171-177 -> torch.optim.Adam / AdamW, optim_base.py:87-89): torch's fused
// kernel deals each launch's tensors out in 64-K-element chunks, one workgroup each, so a 62-M-parameter model
// (SwinUNETR) runs ~1000 workgroups over 16 launches at ~1 TB/s (1.8 ms of the C3 step). Here every workgroup takes
// ADAM_CHUNK elements, so the grid covers the chip and the update streams near the HBM rate (28 bytes per parameter:
// read p, g, m, v, write p, m, v). Round 6: 4096 elements per workgroup as four 1-KB-per-wave groups, all 16 loads of a
// thread issued before the arithmetic, and the bias corrections (f64 pow) evaluated once per workgroup. The arithmetic follows torch's FusedAdamMathFunctor (ATen fused_adam_utils.cuh): the
// moment updates in f64 from f32 operands, bias corrections from the device step count (f64 pow, kept in f32),
// step size and denominator rounded to f32, the final update in f32 -- so results match torch's fused Adam.
//
// LR schedules (lci_adam_step_ex): the workgroup's thread that evaluates the bias corrections also picks this update's
// learning rate and beta1 -- the launch constants, a one-element device tensor (torch's tensor-lr convention: StepLR /
// ReduceLROnPlateau fill_ it and a captured step sees the change), or torch's two-phase cosine OneCycleLR evaluated at
// the tensor's own device step count (trainer_base.py:181-182, optim_base.py:113-115; cycle_momentum cycles beta1) --
// and hands them to the other threads through LDS next to the two coefficients. A captured step therefore follows the
// schedule with no extra launch and no host value baked into the graph. An optional device clip coefficient
// (lci_grad_sumsq + lci_grad_clip_coef: clip_grad_norm_'s norm and coefficient, trainer_base.py:173-175, without
// atomics) multiplies every gradient in f32 first, which saves clip_grad_norm_'s read-modify-write of the gradients.
#include "common.hpp"

namespace lci {

constexpr int ADAM_MAXT = 40;       // tensors per launch (kernel-argument space)
constexpr int ADAM_CHUNK = 4096;    // elements per workgroup (256 threads x 4 groups of 4)

struct AdamTensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  const float* step;   // this tensor's step count (already incremented for this update)
  long long n;
};

struct AdamArgs {
  AdamTensor t[ADAM_MAXT];
  int blk0[ADAM_MAXT + 1];   // first workgroup of each tensor (prefix sums), blk0[nt] = grid size
  int nt;
  double lr, beta1, beta2, wd, eps;
  int adamw, maximize;
  const float* lr_dev;   // optional: the learning rate as one device f32
  const float* gcoef;    // optional: every gradient is multiplied by this device f32 first
  int has_sched;         // sched[] holds a one-cycle schedule
  double sched[8];       // total_steps, end_step1, initial_lr, max_lr, min_lr, base_momentum, max_momentum, 0
};

// torch's OneCycleLR.get_lr (two phases, cosine annealing, cycle_momentum) at step_num, in torch's operation order
// and without FP contraction: cos is the only operation that can differ from the host's.
__device__ __forceinline__ double onecycle_anneal(double start, double end, double q) {
#pragma clang fp contract(off)
  const double cos_out = cos(3.141592653589793 * q) + 1.0;
  return end + (start - end) / 2.0 * cos_out;
}

__device__ __forceinline__ void onecycle(const double* s, double step_num, double& lr, double& beta1) {
#pragma clang fp contract(off)
  const double total = s[0], end1 = s[1];
  if (step_num <= end1) {
    const double q = (step_num - 0.0) / (end1 - 0.0);
    lr = onecycle_anneal(s[2], s[3], q);
    beta1 = onecycle_anneal(s[6], s[5], q);
  } else {
    const double q = (step_num - end1) / ((total - 1.0) - end1);
    lr = onecycle_anneal(s[3], s[4], q);
    beta1 = onecycle_anneal(s[5], s[6], q);
  }
}

template <bool EX>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamArgs& a, double lr,
                                          double beta1, float gc, float step_size, float bc2s) {
  if (EX && a.gcoef) g *= gc;
  float grad = a.maximize ? -g : g;
  if (a.wd != 0.0) {
    if (a.adamw) p = (float)((double)p - lr * a.wd * (double)p);
    else grad = (float)((double)grad + (double)p * a.wd);
  }
  m = (float)(beta1 * (double)m + (1.0 - beta1) * (double)grad);
  v = (float)(a.beta2 * (double)v + (1.0 - a.beta2) * (double)grad * (double)grad);
  const float denom = (float)((double)(sqrtf(v) / bc2s) + a.eps);
  p -= step_size * m / denom;
}

// EX = false: the constant-hyper-parameter update (lci_adam_step): learning rate and beta1 are the launch constants.
// EX = true (any optional input of lci_adam_step_ex): thread 0 picks them per workgroup and shares them through LDS.
template <bool EX>
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
  const int b = blockIdx.x;
  int k = 0;
  while (k + 1 < a.nt && a.blk0[k + 1] <= b) ++k;   // this workgroup's tensor (uniform)
  const AdamTensor& t = a.t[k];
  const long long e0 = (long long)(b - a.blk0[k]) * ADAM_CHUNK;
  __shared__ float coef[3];
  __shared__ double hyp[2];
  float step_size, bc2s, gc = 1.0f;
  double lr = a.lr, beta1 = a.beta1;
  // thread 0 evaluates the workgroup's hyper-parameters and coefficients; everyone picks them up after the barrier
  auto hyper = [&]() {
    if (threadIdx.x == 0) {
      const float stp = *t.step;
      double lr0 = a.lr, beta10 = a.beta1;
      if (EX) {
        if (a.has_sched) onecycle(a.sched, (double)stp - 1.0, lr0, beta10);
        else if (a.lr_dev) lr0 = (double)*a.lr_dev;
        coef[2] = a.gcoef ? *a.gcoef : 1.0f;                        // gradient clip coefficient
        hyp[0] = lr0;
        hyp[1] = beta10;
      }
      const float bc1 = (float)(1.0 - pow(beta10, (double)stp));
      coef[0] = (float)(lr0 / (double)bc1);                         // step size
      coef[1] = (float)sqrt(1.0 - pow(a.beta2, (double)stp));       // sqrt(bias correction 2)
    }
    __syncthreads();
    step_size = coef[0];
    bc2s = coef[1];
    if (EX) {
      gc = coef[2];
      lr = hyp[0];
      beta1 = hyp[1];
    }
  };
  if (!EX) hyper();
  const bool vec = (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0;
  const long long i0 = e0 + 4LL * threadIdx.x;   // group h: elements i0 + 1024 h .. + 3
  if (vec && e0 + ADAM_CHUNK <= t.n) {
    f32x4 p[4], g[4], m[4], v[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const long long i = i0 + 1024 * h;
      p[h] = *(const f32x4*)(t.p + i); g[h] = *(const f32x4*)(t.g + i);
      m[h] = *(const f32x4*)(t.m + i); v[h] = *(const f32x4*)(t.v + i);
    }
    if (EX) hyper();   // the schedule's cos and the two pows run under the 16 loads just issued (a uniform branch)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const long long i = i0 + 1024 * h;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[h][j], mj = m[h][j], vj = v[h][j];
        adam_elem<EX>(pj, g[h][j], mj, vj, a, lr, beta1, gc, step_size, bc2s);
        p[h][j] = pj; m[h][j] = mj; v[h][j] = vj;
      }
      *(f32x4*)(t.p + i) = p[h];
      *(f32x4*)(t.m + i) = m[h];
      *(f32x4*)(t.v + i) = v[h];
    }
  } else {
    if (EX) hyper();
    for (int h = 0; h < 4; ++h)
      for (long long i = i0 + 1024 * h; i < i0 + 1024 * h + 4 && i < t.n; ++i) {
        float p = t.p[i], m = t.m[i], v = t.v[i];
        adam_elem<EX>(p, t.g[i], m, v, a, lr, beta1, gc, step_size, bc2s);
        t.p[i] = p; t.m[i] = m; t.v[i] = v;
      }
  }
}

struct OneCycleArgs {
  double sched[8];   // as AdamArgs::sched
};

__global__ __launch_bounds__(256) void onecycle_eval_kernel(const float* __restrict__ step, int n, OneCycleArgs a,
                                                            double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double lr, beta1;
  onecycle(a.sched, (double)step[i] - 1.0, lr, beta1);
  out[2 * i] = lr;
  out[2 * i + 1] = beta1;
}

// Sum of a workgroup's 256 f64 values in a fixed order (lane tree per wave, then the four waves in order); the
// result is valid in thread 0.
__device__ __forceinline__ double block_sum256(double s, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

struct SumsqArgs {
  const float* g[ADAM_MAXT];
  long long n[ADAM_MAXT];
  int blk0[ADAM_MAXT + 1];
  int nt;
  double* part;   // one partial per workgroup
};

// One partial sum of squares (f64 accumulation of f32 gradients) per ADAM_CHUNK elements, adam_kernel's partition.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(SumsqArgs a) {
  const int b = blockIdx.x;
  int k = 0;
  while (k + 1 < a.nt && a.blk0[k + 1] <= b) ++k;
  const float* g = a.g[k];
  const long long n = a.n[k];
  const long long e0 = (long long)(b - a.blk0[k]) * ADAM_CHUNK;
  const long long i0 = e0 + 4LL * threadIdx.x;
  double s = 0.0;
  if ((((uintptr_t)g) & 15) == 0 && e0 + ADAM_CHUNK <= n) {
    f32x4 x[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) x[h] = *(const f32x4*)(g + i0 + 1024 * h);
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) s += (double)x[h][j] * (double)x[h][j];
  } else {
    for (int h = 0; h < 4; ++h)
      for (long long i = i0 + 1024 * h; i < i0 + 1024 * h + 4 && i < n; ++i) s += (double)g[i] * (double)g[i];
  }
  __shared__ double red[4];
  const double tot = block_sum256(s, red);
  if (threadIdx.x == 0) a.part[b] = tot;
}

// clip_grad_norm_'s total norm and clip coefficient from the partials, summed in a fixed order.
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const double* __restrict__ part, long long nparts,
                                                             float max_norm, float* __restrict__ out) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < nparts; i += 256) s += part[i];
  __shared__ double red[4];
  const double tot = block_sum256(s, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(tot);
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.0f ? 1.0f : c;   // a NaN norm keeps its NaN (torch.clamp), an inf norm gives 0
  }
}

}  // namespace lci

using namespace lci;

extern "C" int lci_adam_max_tensors(void) { return ADAM_MAXT; }

static int adam_launch(float* const* p, const float* const* g, float* const* m, float* const* v,
                       const float* const* step, const long long* n, int nt, double lr, double beta1, double beta2,
                       double weight_decay, double eps, int adamw, int maximize, const float* lr_dev,
                       const double* sched, const float* gcoef, void* stream) {
  LCI_CHECK(nt >= 1 && nt <= ADAM_MAXT, "adam_step: %d tensors (1 .. %d per call)", nt, ADAM_MAXT);
  LCI_CHECK(!(sched && lr_dev), "adam_step: a one-cycle schedule and a device learning rate exclude each other");
  AdamArgs a{};
  long long blocks = 0;
  for (int i = 0; i < nt; ++i) {
    LCI_CHECK(n[i] >= 0 && p[i] && g[i] && m[i] && v[i] && step[i], "adam_step: tensor %d: null pointer or bad size", i);
    a.t[i] = AdamTensor{p[i], g[i], m[i], v[i], step[i], n[i]};
    a.blk0[i] = (int)blocks;
    blocks += (n[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    LCI_CHECK(blocks < (1LL << 31), "adam_step: too many elements in one call");
  }
  a.blk0[nt] = (int)blocks;
  a.nt = nt;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.wd = weight_decay; a.eps = eps;
  a.adamw = adamw; a.maximize = maximize;
  a.lr_dev = lr_dev; a.gcoef = gcoef;
  if (sched) {
    LCI_CHECK(sched[0] >= 1.0, "adam_step: one-cycle schedule of %g steps", sched[0]);
    a.has_sched = 1;
    for (int i = 0; i < 8; ++i) a.sched[i] = sched[i];
  }
  if (blocks == 0) return 0;
  if (lr_dev || sched || gcoef)
    hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  LCI_LAUNCH_CHECK();
  return 0;
}

extern "C" int lci_adam_step(float* const* p, const float* const* g, float* const* m, float* const* v,
                             const float* const* step, const long long* n, int nt, double lr, double beta1,
                             double beta2, double weight_decay, double eps, int adamw, int maximize, void* stream) {
  return adam_launch(p, g, m, v, step, n, nt, lr, beta1, beta2, weight_decay, eps, adamw, maximize, nullptr, nullptr,
                     nullptr, stream);
}

extern "C" int lci_adam_step_ex(float* const* p, const float* const* g, float* const* m, float* const* v,
                                const float* const* step, const long long* n, int nt, double lr, double beta1,
                                double beta2, double weight_decay, double eps, int adamw, int maximize,
                                const float* lr_dev, const double* sched, const float* gcoef, void* stream) {
  return adam_launch(p, g, m, v, step, n, nt, lr, beta1, beta2, weight_decay, eps, adamw, maximize, lr_dev, sched,
                     gcoef, stream);
}

extern "C" int lci_onecycle_eval(const float* step, int n, const double* sched, double* out, void* stream) {
  LCI_CHECK(n >= 0 && sched && (n == 0 || (step && out)), "onecycle_eval: null pointer or bad size");
  LCI_CHECK(sched[0] >= 1.0, "onecycle_eval: one-cycle schedule of %g steps", sched[0]);
  if (n == 0) return 0;
  OneCycleArgs a{};
  for (int i = 0; i < 8; ++i) a.sched[i] = sched[i];
  hipLaunchKernelGGL(onecycle_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, step,
                     n, a, out);
  LCI_LAUNCH_CHECK();
  return 0;
}

extern "C" long long lci_grad_sumsq_parts(const long long* n, int nt) {
  long long blocks = 0;
  for (int i = 0; i < nt; ++i) {
    if (n[i] < 0) return -1;
    blocks += (n[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
  }
  return blocks;
}

extern "C" int lci_grad_sumsq(const float* const* g, const long long* n, int nt, double* part, void* stream) {
  LCI_CHECK(nt >= 1 && nt <= ADAM_MAXT, "grad_sumsq: %d tensors (1 .. %d per call)", nt, ADAM_MAXT);
  SumsqArgs a{};
  long long blocks = 0;
  for (int i = 0; i < nt; ++i) {
    LCI_CHECK(n[i] >= 0 && g[i], "grad_sumsq: tensor %d: null pointer or bad size", i);
    a.g[i] = g[i];
    a.n[i] = n[i];
    a.blk0[i] = (int)blocks;
    blocks += (n[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    LCI_CHECK(blocks < (1LL << 31), "grad_sumsq: too many elements in one call");
  }
  a.blk0[nt] = (int)blocks;
  a.nt = nt;
  if (blocks == 0) return 0;
  LCI_CHECK(part, "grad_sumsq: null workspace");
  a.part = part;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  LCI_LAUNCH_CHECK();
  return 0;
}

extern "C" int lci_grad_clip_coef(const double* part, long long nparts, double max_norm, float* out, void* stream) {
  LCI_CHECK(nparts >= 0 && out && (nparts == 0 || part), "grad_clip_coef: null pointer or bad size");
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nparts,
                     (float)max_norm, out);
  LCI_LAUNCH_CHECK();
  return 0;
}
