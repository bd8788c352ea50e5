// Evaluation tally: top-1 / top-k hit counts and the summed cross-entropy of a batch of logits, optionally restricted
// to a class subset, in one pass over the logits (reference src/evaluation/metrics.py:19-55: outputs[:, valid_indices],
// MulticlassAccuracy(top_k = 1 | 5), criterion(outputs, labels)).  Per row b, with z_j = logits[b, keep[j]] (keep NULL:
// z_j = logits[b, j]), y = labels[b] an index into the SUBSET and s the label smoothing, everything in fp64 on the
// values as stored:
//     rank = #{j : z_j > z_y} + #{j < y : z_j == z_y}      (a tie goes to the lowest subset position, like argmax;
//                                                           NaN orders above every number and equal to NaN, like topk)
//     loss = lse(z) - (1 - s) z_y - (s / K) sum_j z_j      (the last term only when s != 0, so that a -inf logit away
//                                                           from the target is legal at s = 0, as in torch)
//     lse(z) = m + log(sum_j exp(z_j - m)),  m = the largest non-NaN z_j, 0 where that is infinite.
// A label outside [0, K) reads nothing: rank = K (a miss at every k) and loss = NaN.  A keep entry outside [0, C) reads
// nothing either: its z_j counts as NaN.
// Two launches: one 256-thread workgroup per row writes row_rank / row_loss; one workgroup then sums them over b in a
// fixed order (thread t takes b = t, t + 256, ... in turn, xor-butterfly over the 64 lanes, the four waves left to
// right) and adds {hits@1, hits@top_k, summed loss, B} to the caller's four doubles.  No floating-point atomics: the
// tally is bitwise reproducible.  torch runs about a dozen launches for this, a sort among them.
#include "basd_common.h"

#include <math.h>

namespace basd {

// the four waves through LDS; every thread gets the result
__device__ __forceinline__ double tally_block_sum(double v, double* red) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double tally_block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

template <bool BF16>
__device__ __forceinline__ double tally_load(const void* row, int64_t col) {
  if (BF16) return (double)bf16_bits_to_f32(((const unsigned short*)row)[col]);
  return (double)((const float*)row)[col];
}

// z_j of the row, NaN for a keep entry that points outside the row
template <bool BF16>
__device__ __forceinline__ double tally_subset_load(const void* row, const int64_t* __restrict__ keep, int j, int C) {
  int64_t col = j;
  if (keep) {
    col = keep[j];
    if (col < 0 || col >= C) return (double)NAN;
  }
  return tally_load<BF16>(row, col);
}

template <bool BF16>
__global__ __launch_bounds__(256) void cls_tally_rows_kernel(const void* __restrict__ logits, int64_t row_stride,
                                                             const int64_t* __restrict__ labels,
                                                             const int64_t* __restrict__ keep, int C, int K,
                                                             double smoothing, int* __restrict__ row_rank,
                                                             double* __restrict__ row_loss) {
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t lab = labels[b];
  if (lab < 0 || lab >= K) {                       // uniform over the workgroup: nobody reaches a barrier
    if (tid == 0) {
      row_rank[b] = K;
      row_loss[b] = (double)NAN;
    }
    return;
  }
  const int y = (int)lab;
  const void* row = BF16 ? (const void*)((const unsigned short*)logits + (int64_t)b * row_stride)
                         : (const void*)((const float*)logits + (int64_t)b * row_stride);
  const double zy = tally_subset_load<BF16>(row, keep, y, C);
  const bool zy_nan = zy != zy;
  double mx = -INFINITY, sz = 0.0;
  int above = 0;
  for (int j = tid; j < K; j += 256) {
    const double z = tally_subset_load<BF16>(row, keep, j, C);
    const bool z_nan = z != z;
    mx = fmax(mx, z);                                // fmax drops a NaN operand
    sz += z;
    const bool gt = z_nan ? !zy_nan : z > zy;        // z > NaN is false
    const bool eq = z_nan ? zy_nan : z == zy;
    above += (gt || (eq && j < y)) ? 1 : 0;
  }
  mx = tally_block_max(mx, red);
  if (isinf(mx)) mx = 0.0;                           // all -inf, or a +inf: exp(z - 0) keeps the infinities' meaning
  double se = 0.0;
  for (int j = tid; j < K; j += 256) se += exp(tally_subset_load<BF16>(row, keep, j, C) - mx);
  se = tally_block_sum(se, red);
  const int rank = (int)tally_block_sum((double)above, red);          // <= K < 2^31: exact in a double
  double loss = mx + log(se) - (1.0 - smoothing) * zy;
  if (smoothing != 0.0) loss -= smoothing / (double)K * tally_block_sum(sz, red);
  if (tid == 0) {
    row_rank[b] = rank;
    row_loss[b] = loss;
  }
}

__global__ __launch_bounds__(256) void cls_tally_finish_kernel(const int* __restrict__ row_rank,
                                                               const double* __restrict__ row_loss, int B, int top_k,
                                                               double* __restrict__ tally) {
  __shared__ double red[4];
  double h1 = 0.0, hk = 0.0, ls = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const int r = row_rank[b];
    h1 += r == 0 ? 1.0 : 0.0;
    hk += r < top_k ? 1.0 : 0.0;
    ls += row_loss[b];
  }
  h1 = tally_block_sum(h1, red);
  hk = tally_block_sum(hk, red);
  ls = tally_block_sum(ls, red);
  if (threadIdx.x == 0) {
    tally[0] += h1;
    tally[1] += hk;
    tally[2] += ls;
    tally[3] += (double)B;
  }
}

}  // namespace basd

extern "C" int basd_cls_tally(const void* logits, int logits_bf16, int64_t row_stride, const int64_t* labels,
                              const int64_t* keep, int B, int C, int K, int top_k, float smoothing, int* row_rank,
                              double* row_loss, double* tally, void* stream) {
  using namespace basd;
  if (B == 0) return BASD_OK;
  if (B < 0 || C <= 0 || K <= 0) return fail(BASD_ERR_SHAPE, "cls_tally: B %d, C %d, K %d must be positive", B, C, K);
  if (keep == nullptr && K != C)
    return fail(BASD_ERR_SHAPE, "cls_tally: without a keep list K (%d) must equal C (%d)", K, C);
  if (top_k < 1 || top_k > K) return fail(BASD_ERR_SHAPE, "cls_tally: top_k %d outside 1 .. K = %d", top_k, K);
  if (row_stride < C)
    return fail(BASD_ERR_SHAPE, "cls_tally: row_stride %lld is smaller than C = %d", (long long)row_stride, C);
  if (logits == nullptr || labels == nullptr)
    return fail(BASD_ERR_SHAPE, "cls_tally: logits [B, C] and labels [B] are required");
  if (row_rank == nullptr || row_loss == nullptr || tally == nullptr)
    return fail(BASD_ERR_SHAPE, "cls_tally: row_rank [B], row_loss [B] and tally [4] are required");
  hipStream_t st = (hipStream_t)stream;
  if (logits_bf16)
    hipLaunchKernelGGL(cls_tally_rows_kernel<true>, dim3(B), dim3(256), 0, st, logits, row_stride, labels, keep, C, K,
                       (double)smoothing, row_rank, row_loss);
  else
    hipLaunchKernelGGL(cls_tally_rows_kernel<false>, dim3(B), dim3(256), 0, st, logits, row_stride, labels, keep, C, K,
                       (double)smoothing, row_rank, row_loss);
  hipLaunchKernelGGL(cls_tally_finish_kernel, dim3(1), dim3(256), 0, st, row_rank, row_loss, B, top_k, tally);
  return check_launch("cls_tally");
}
