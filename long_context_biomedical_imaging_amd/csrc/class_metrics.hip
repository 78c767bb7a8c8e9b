// Classification metrics of the reference's step tail (metrics/metrics_base.py:59-78, 157-160, 268-285, 304-376):
// acc_1, AUROC and F1 of softmax scores, per step or exactly over a whole evaluation epoch, left in device memory
// (the reference runs torchmetrics on a host-visible list of tensors and a sort-based f32 ROC curve).
//
// Scores p = softmax(logits (B, C), dim 1) evaluated in f64 and rounded once to f32. K score columns are kept:
// K = 1 for C == 2 (the 'binary' task: p[:, 1], positive class 1), K = C otherwise (one-vs-rest per column).
//
//   cm_softmax   one thread per row: row b -> probs[base + b] (K columns) and labels[base + b], base = *count (0 for
//                the per-step op). Rows at or past `capacity` are dropped. A row's arithmetic is a sequential loop over
//                its own C logits, so identical rows give identical bits wherever they land.
//   cm_bump      one thread: *count += B, after every cm_softmax thread read the old value (stream order), so a
//                captured append replays correctly.
//   cm_count     per row the prediction (binary: score > 0.5; multiclass: first maximum of the stored row) and
//                tp / fp / fn / P per class plus the correct predictions, in LDS u32 counters, then one u64 integer
//                atomic per non-zero counter and workgroup.
//   cm_pairs     U2[c] = sum over positives i and negatives j of 2 [s_i > s_j] + [s_i == s_j] on the stored f32
//                scores. Grid (i chunks, K, j splits): a workgroup compacts the positives of class c among its CM_TI
//                rows i into LDS, so no lane compares for a row that is no positive (1 / C of the rows for balanced
//                classes); a thread owns one positive per batch of 256. CM_TJ rows of column c go to LDS per tile
//                with the positives and the tail replaced by NaN (every comparison false), counted in u32 per
//                thread, reduced per wave and workgroup in u64, one u64 integer atomic per workgroup.
//   cm_finalize  Q = n - P, auroc_c = U2 / (2 P Q) (0 when P Q == 0), the mean over the K columns, f1 and acc_1 in f64.
// Integer atomics only: every output is bitwise reproducible. No host sync.
#include "common.hpp"

#include <math.h>

namespace lci {

constexpr int CM_THREADS = 256;
constexpr int CM_TI = 2048;                                      // i rows per workgroup of cm_pairs
constexpr int CM_TJ = 1024;                                      // j rows per LDS tile
constexpr int CM_MAXC = 64;
constexpr int CM_NCNT = 6;                                       // tp, fp, fn, P, Q, U2
constexpr int CM_COUNT_WGS = 1024;
constexpr int CM_PAIR_WGS = 2048;                                // j splits aim at this many workgroups
constexpr int CM_MAX_SPLITS = 64;

__device__ __forceinline__ double cm_ld(const float* p, long long i) { return (double)p[i]; }
__device__ __forceinline__ double cm_ld(const bf16* p, long long i) { return (double)(float)p[i]; }

template <typename TL>
__global__ __launch_bounds__(CM_THREADS) void cm_softmax(const TL* __restrict__ logits,
                                                         const long long* __restrict__ labels,
                                                         float* __restrict__ probs, long long* __restrict__ lab_out,
                                                         const long long* __restrict__ count, long long capacity,
                                                         int B, int C) {
  const int b = blockIdx.x * CM_THREADS + threadIdx.x;
  if (b >= B) return;
  const long long base = count ? *count : 0;
  const long long dst = base + b;
  if (base < 0 || dst >= capacity) return;
  const TL* row = logits + (long long)b * C;
  double m = cm_ld(row, 0);
  for (int c = 1; c < C; ++c) m = fmax(m, cm_ld(row, c));
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += exp(cm_ld(row, c) - m);
  if (C == 2) {
    probs[dst] = (float)(exp(cm_ld(row, 1) - m) / s);
  } else {
    float* o = probs + dst * C;
    for (int c = 0; c < C; ++c) o[c] = (float)(exp(cm_ld(row, c) - m) / s);
  }
  lab_out[dst] = labels[b];
}

__global__ void cm_bump(long long* __restrict__ count, long long B) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *count += B;
}

// counts: (K, 6) u64 followed by the number of correct predictions; zeroed before this kernel.
__global__ __launch_bounds__(CM_THREADS) void cm_count(const float* __restrict__ probs,
                                                       const long long* __restrict__ labels,
                                                       unsigned long long* __restrict__ counts, long long n, int K,
                                                       int C) {
  __shared__ unsigned cnt[4 * CM_MAXC + 1];                      // tp | fp | fn | P per class, then correct
  const int tid = threadIdx.x;
  for (int i = tid; i < 4 * K + 1; i += CM_THREADS) cnt[i] = 0u;
  __syncthreads();
  for (long long r = (long long)blockIdx.x * CM_THREADS + tid; r < n; r += (long long)gridDim.x * CM_THREADS) {
    const long long l = labels[r];
    if (K == 1) {
      const bool pred = probs[r] > 0.5f, pos = l == 1;
      if (pos) atomicAdd(&cnt[3], 1u);
      if (pred && pos) atomicAdd(&cnt[0], 1u);
      if (pred && !pos) atomicAdd(&cnt[1], 1u);
      if (!pred && pos) atomicAdd(&cnt[2], 1u);
      if ((pred && pos) || (!pred && l == 0)) atomicAdd(&cnt[4], 1u);
    } else {
      const float* row = probs + r * K;
      float best = row[0];
      int pred = 0;
      for (int c = 1; c < K; ++c) {
        const float v = row[c];
        if (v > best || (v != v && best == best)) { best = v; pred = c; }   // first maximum; a NaN is a maximum
      }
      const bool in = l >= 0 && l < C;
      if (in) atomicAdd(&cnt[3 * K + (int)l], 1u);
      if (l == pred) {
        atomicAdd(&cnt[pred], 1u);
        atomicAdd(&cnt[4 * K], 1u);
      } else {
        atomicAdd(&cnt[K + pred], 1u);
        if (in) atomicAdd(&cnt[2 * K + (int)l], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 4 * K + 1; i += CM_THREADS) {
    const unsigned v = cnt[i];
    if (v) atomicAdd(&counts[i == 4 * K ? (long long)CM_NCNT * K : (long long)(i % K) * CM_NCNT + i / K],
                     (unsigned long long)v);
  }
}

// Grid (i chunks, K, splits). A positive meets at most n < 2^31 rows j, and a thread's u32 counts are added to its u64
// sum after each of its positives, so they cannot wrap.
__global__ __launch_bounds__(CM_THREADS) void cm_pairs(const float* __restrict__ probs,
                                                       const long long* __restrict__ labels,
                                                       unsigned long long* __restrict__ counts, int n, int K,
                                                       int splits) {
  __shared__ __attribute__((aligned(16))) float sj[CM_TJ];
  __shared__ float spos[CM_TI];
  __shared__ unsigned npos;
  __shared__ unsigned long long red[CM_THREADS / 64];
  const int tid = threadIdx.x, c = blockIdx.y;
  const long long posc = K == 1 ? 1 : c;
  if (tid == 0) npos = 0u;
  __syncthreads();
  // the chunk's positives of class c, compacted (their order does not matter: integer sums)
  const long long i0 = (long long)blockIdx.x * CM_TI;
  for (int x = tid; x < CM_TI; x += CM_THREADS) {
    const long long i = i0 + x;
    if (i < n && labels[i] == posc) spos[atomicAdd(&npos, 1u)] = probs[i * K + c];
  }
  __syncthreads();
  const int np = (int)npos;
  if (np == 0) return;                                           // the whole workgroup: no barrier is left behind
  unsigned long long u2 = 0ull;
  const int ntiles = (n + CM_TJ - 1) / CM_TJ;
  for (int b0 = 0; b0 < np; b0 += CM_THREADS) {
    const bool mine = b0 + tid < np;
    const float si = mine ? spos[b0 + tid] : NAN;                // NaN: every comparison is false
    const bool work = __ballot(mine) != 0ull;                    // wave-uniform
    unsigned gt = 0u, eq = 0u;
    for (int t = blockIdx.z; t < ntiles; t += splits) {
      __syncthreads();                                           // the previous tile has been read
      for (int x = tid; x < CM_TJ; x += CM_THREADS) {
        const long long j = (long long)t * CM_TJ + x;
        float v = NAN;
        if (j < n && labels[j] != posc) v = probs[j * K + c];
        sj[x] = v;
      }
      __syncthreads();
      if (work) {
#pragma unroll 4
        for (int x = 0; x < CM_TJ; x += 4) {
          const f32x4 v = *(const f32x4*)(sj + x);
          gt += (unsigned)(si > v[0]) + (unsigned)(si > v[1]) + (unsigned)(si > v[2]) + (unsigned)(si > v[3]);
          eq += (unsigned)(si == v[0]) + (unsigned)(si == v[1]) + (unsigned)(si == v[2]) + (unsigned)(si == v[3]);
        }
      }
    }
    u2 += 2ull * gt + eq;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) u2 += __shfl_xor(u2, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = u2;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long tot = (red[0] + red[1]) + (red[2] + red[3]);
    if (tot) atomicAdd(&counts[(long long)c * CM_NCNT + 5], tot);
  }
}

// result[3] f64 = acc_1, auroc, f1.
__global__ void cm_finalize(long long* __restrict__ counts, double* __restrict__ result, long long n, int K) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double auroc = 0.0, f1 = 0.0;
  int present = 0;
  for (int c = 0; c < K; ++c) {
    long long* q = counts + (long long)c * CM_NCNT;
    const long long P = q[3], Q = n - P;
    q[4] = Q;
    if (P > 0 && Q > 0) auroc += (double)q[5] / (2.0 * (double)P * (double)Q);
    const double tp = (double)q[0], d = 2.0 * tp + (double)q[1] + (double)q[2];
    if (d > 0.0) { f1 += 2.0 * tp / d; ++present; }
  }
  result[0] = (double)counts[(long long)CM_NCNT * K] / (double)n;
  result[1] = auroc / K;
  result[2] = K == 1 ? f1 : (present > 0 ? f1 / present : 0.0);   // binary: class 1; else macro over present classes
}

static int cm_splits(long long n, int K) {
  const long long itiles = (n + CM_TI - 1) / CM_TI, jtiles = (n + CM_TJ - 1) / CM_TJ;
  long long s = CM_PAIR_WGS / (itiles * K);
  if (s > jtiles) s = jtiles;
  if (s > CM_MAX_SPLITS) s = CM_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

static int cm_score_launch(const float* probs, const long long* labels, long long* counts, double* result,
                           long long n, int C, hipStream_t st) {
  const int K = C == 2 ? 1 : C;
  LCI_HIP(hipMemsetAsync(counts, 0, (size_t)(CM_NCNT * K + 1) * 8, st));
  long long wgs = (n + CM_THREADS - 1) / CM_THREADS;
  if (wgs > CM_COUNT_WGS) wgs = CM_COUNT_WGS;
  hipLaunchKernelGGL(cm_count, dim3((unsigned)wgs), dim3(CM_THREADS), 0, st, probs, labels,
                     (unsigned long long*)counts, n, K, C);
  LCI_LAUNCH_CHECK();
  const int splits = cm_splits(n, K);
  hipLaunchKernelGGL(cm_pairs, dim3((unsigned)((n + CM_TI - 1) / CM_TI), (unsigned)K, (unsigned)splits),
                     dim3(CM_THREADS), 0, st, probs, labels, (unsigned long long*)counts, (int)n, K, splits);
  LCI_LAUNCH_CHECK();
  hipLaunchKernelGGL(cm_finalize, dim3(1), dim3(64), 0, st, counts, result, n, K);
  LCI_LAUNCH_CHECK();
  return 0;
}

template <typename TL>
static int cm_softmax_launch(const void* logits, const long long* labels, float* probs, long long* lab_out,
                             const long long* count, long long capacity, int B, int C, hipStream_t st) {
  hipLaunchKernelGGL((cm_softmax<TL>), dim3((unsigned)((B + CM_THREADS - 1) / CM_THREADS)), dim3(CM_THREADS), 0, st,
                     (const TL*)logits, labels, probs, lab_out, count, capacity, B, C);
  LCI_LAUNCH_CHECK();
  return 0;
}

static long long cm_align16(long long b) { return (b + 15) / 16 * 16; }

}  // namespace lci

using namespace lci;

extern "C" int lci_class_tile(int axis) { return axis == 0 ? CM_TI : axis == 1 ? CM_TJ : -1; }

extern "C" long long lci_class_metrics_ws_bytes(int B, int C) {
  if (B < 1 || C < 2 || C > CM_MAXC) return -1;
  return cm_align16((long long)B * (C == 2 ? 1 : C) * 4) + (long long)B * 8;
}

extern "C" int lci_class_append(const void* logits, int dtype, const long long* labels, float* probs,
                                long long* label_buf, long long* count, long long capacity, int B, int C,
                                void* stream) {
  LCI_CHECK(B >= 1 && capacity >= 1, "class_append: B = %d, capacity = %lld (both at least 1)", B, capacity);
  LCI_CHECK(C >= 2 && C <= CM_MAXC, "class_append: C = %d outside [2, %d]", C, CM_MAXC);
  LCI_CHECK(dtype == 0 || dtype == 1, "class_append: dtype code %d (0 = f32, 1 = bf16)", dtype);
  LCI_CHECK(logits && labels && probs && label_buf && count, "class_append: null pointer");
  LCI_CHECK(((uintptr_t)labels & 7) == 0 && ((uintptr_t)label_buf & 7) == 0 && ((uintptr_t)count & 7) == 0 &&
                ((uintptr_t)probs & 3) == 0,
            "class_append: labels / label_buf / count must be 8-byte aligned, probs 4-byte");
  hipStream_t st = (hipStream_t)stream;
  const int rc = dtype == 0
      ? cm_softmax_launch<float>(logits, labels, probs, label_buf, count, capacity, B, C, st)
      : cm_softmax_launch<bf16>(logits, labels, probs, label_buf, count, capacity, B, C, st);
  if (rc) return rc;
  hipLaunchKernelGGL(cm_bump, dim3(1), dim3(64), 0, st, count, (long long)B);
  LCI_LAUNCH_CHECK();
  return 0;
}

extern "C" int lci_class_score(const float* probs, const long long* labels, long long* counts, double* result,
                               long long n, int C, void* stream) {
  LCI_CHECK(n >= 1 && n < (1LL << 31), "class_score: n = %lld outside [1, 2^31)", n);
  LCI_CHECK(C >= 2 && C <= CM_MAXC, "class_score: C = %d outside [2, %d]", C, CM_MAXC);
  LCI_CHECK(probs && labels && counts && result, "class_score: null pointer");
  LCI_CHECK(((uintptr_t)labels & 7) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)result & 7) == 0 &&
                ((uintptr_t)probs & 3) == 0,
            "class_score: labels / counts / result must be 8-byte aligned, probs 4-byte");
  return cm_score_launch(probs, labels, counts, result, n, C, (hipStream_t)stream);
}

extern "C" int lci_class_metrics(const void* logits, int dtype, const long long* labels, long long* counts,
                                 double* result, void* ws, int B, int C, void* stream) {
  LCI_CHECK(B >= 1, "class_metrics: B = %d", B);
  LCI_CHECK(C >= 2 && C <= CM_MAXC, "class_metrics: C = %d outside [2, %d]", C, CM_MAXC);
  LCI_CHECK(dtype == 0 || dtype == 1, "class_metrics: dtype code %d (0 = f32, 1 = bf16)", dtype);
  LCI_CHECK(logits && labels && counts && result && ws, "class_metrics: null pointer");
  LCI_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)counts & 7) == 0 &&
                ((uintptr_t)result & 7) == 0,
            "class_metrics: ws must be 16-byte aligned, labels / counts / result 8-byte");
  hipStream_t st = (hipStream_t)stream;
  float* probs = (float*)ws;
  long long* lab = (long long*)((char*)ws + cm_align16((long long)B * (C == 2 ? 1 : C) * 4));
  const int rc = dtype == 0
      ? cm_softmax_launch<float>(logits, labels, probs, lab, nullptr, (long long)B, B, C, st)
      : cm_softmax_launch<bf16>(logits, labels, probs, lab, nullptr, (long long)B, B, C, st);
  if (rc) return rc;
  return cm_score_launch(probs, lab, counts, result, B, C, st);
}
