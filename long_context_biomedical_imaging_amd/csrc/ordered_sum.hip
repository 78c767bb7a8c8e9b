// Ordered sum of partial rows: the second half of the store-and-sum form the deterministic mode uses in place of
// float atomics (mamba.hip, hyena.hip, patch_embed.hip). Every contributor has stored its partial once with plain
// stores; this launch produces
//     out[c] = sum_r part[r * row_stride + c * col_stride],   c < n, r < rows
// with one writer per out[c] and an order of additions that depends on `rows` alone, so equal inputs give equal bits.
//
// Tree: the rows are dealt round-robin to RS slices (RS = 1 for rows <= 8, 4 below 256 rows, 16 from there on). A
// slice adds its rows in increasing order into four accumulators (rows s + RS (4 i + k) into accumulator k, the
// remainder of fewer than four rows into accumulator 0) and closes with (a0 + a1) + (a2 + a3); the slices are then
// added in slice order. A workgroup is RS slices x 256 / RS adjacent columns, so a wave reads adjacent columns.
#include "common.hpp"

namespace lci {

template <int RS>
__global__ __launch_bounds__(256) void ordered_sum_kernel(const float* __restrict__ part, long long row_stride,
                                                          int col_stride, int rows, long long n,
                                                          float* __restrict__ out) {
  constexpr int CW = 256 / RS;
  __shared__ float sh[256];
  const int cl = threadIdx.x % CW, s = threadIdx.x / CW;
  const long long c = (long long)blockIdx.x * CW + cl;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < n) {
    const float* p = part + c * col_stride;
    int r = s;
    for (; r + 3 * RS < rows; r += 4 * RS) {
      a0 += p[r * row_stride];
      a1 += p[(r + RS) * row_stride];
      a2 += p[(r + 2 * RS) * row_stride];
      a3 += p[(r + 3 * RS) * row_stride];
    }
    for (; r < rows; r += RS) a0 += p[r * row_stride];
  }
  float t = (a0 + a1) + (a2 + a3);
  if (RS > 1) {
    sh[threadIdx.x] = t;
    __syncthreads();
    if (s != 0) return;
#pragma unroll
    for (int k = 1; k < RS; ++k) t += sh[k * CW + cl];
  }
  if (c < n) out[c] = t;
}

int ordered_sum(const float* part, long long row_stride, int col_stride, int rows, long long n, float* out,
                hipStream_t s) {
  LCI_CHECK(part && out && rows > 0 && n > 0 && col_stride > 0 && row_stride >= 0,
            "ordered_sum: bad arguments (rows %d, n %lld)", rows, n);
  const int rs = rows <= 8 ? 1 : (rows < 256 ? 4 : 16);
  const long long blocks = (n + 256 / rs - 1) / (256 / rs);
  LCI_CHECK(blocks < (1ll << 31), "ordered_sum: n %lld too large", n);
  const dim3 grid((unsigned)blocks);
  if (rs == 1) hipLaunchKernelGGL(ordered_sum_kernel<1>, grid, dim3(256), 0, s, part, row_stride, col_stride, rows, n, out);
  else if (rs == 4) hipLaunchKernelGGL(ordered_sum_kernel<4>, grid, dim3(256), 0, s, part, row_stride, col_stride, rows, n, out);
  else hipLaunchKernelGGL(ordered_sum_kernel<16>, grid, dim3(256), 0, s, part, row_stride, col_stride, rows, n, out);
  LCI_LAUNCH_CHECK();
  return 0;
}

}  // namespace lci

extern "C" int lci_ordered_sum(const float* part, long long row_stride, int col_stride, int rows, long long n,
                               float* out, void* stream) {
  return lci::ordered_sum(part, row_stride, col_stride, rows, n, out, (hipStream_t)stream);
}
