// Gradient of the loss with respect to the tapped student token tensors, as two C entries.
//
// basd_selector_token_grad: the selector's share, g_e = bf16((s_e - mean_e) W_e) for all E extraction points in one
// call (two launches).  The tokens are exact bf16 values, so only the fp32 W is split: W = W1 + W2 + W3 in bf16
// (24 significant bits), three bf16-MFMA products per K chunk with fp32 accumulation: the accuracy of an fp32 GEMM
// at a third of the fp32-MFMA cost.  The centring is applied as the torch chain applied it, after the product:
// s W - mean W, with the row -mean W as the initial value of the accumulators.
//   launch 1  column sums of every tap in fp64 (per-workgroup partials, no atomics, no zero fill) and the transposed
//             bf16 splits of W into the workspace
//   launch 2  per workgroup: the mean and the row of its tap (fixed summation order), then tiles of 256 token rows x
//             192 output columns.  W sits in the A operand and the tokens in the B operand of
//             v_mfma_f32_16x16x32_bf16, so that a lane ends up with four consecutive output columns of one token row
//             and stores them as one 8-byte word.  The W chunk of a K step (3 splits x 192 columns x 32 k) is staged in
//             LDS, double buffered, and serves the four row groups of all four waves; it does not fit LDS whole
//             (3 x 72 KiB at 192) and re-reading it from L2 per wave would move 220 KiB per 64 rows.
//
// basd_tap_grad_scatter: what autograd did around the tap out[:, 1:, :] (add of the two view gradients, zero fill,
// strided copy, add into the gradient of the block output) in one pass of 16-byte accesses, with autograd's rounding.
#include "basd_frag.h"

namespace basd {

constexpr int TG_MAX_E = 8;
constexpr int TG_MAX_G = 64;          // column-sum partials per tap
constexpr int TG_ROWS = 256;          // token rows per tile (64 per wave)
constexpr int TG_COLS = 192;          // output columns per tile
constexpr int TG_NCT = TG_COLS / 16;
constexpr int TG_KC = 32;             // K chunk
constexpr int TG_PROW = 80;           // bytes per (split, column) row of a staged W chunk (64 + 16 pad)
constexpr int TG_MAX_D = 768;
constexpr size_t TG_PBUF = (size_t)3 * TG_COLS * TG_PROW;

struct TapPtrs {
  const unsigned short* s[TG_MAX_E];
  unsigned short* out[TG_MAX_E];
};

static int tg_partials(int64_t rows) {
  int64_t g = (rows + 127) / 128;
  return (int)(g < 1 ? 1 : g > TG_MAX_G ? TG_MAX_G : g);
}

// launch 1: workgroups [0, E * G) sum a slab of rows of one tap; the rest split W.
__global__ __launch_bounds__(256) void tap_colsum_split_kernel(TapPtrs tp, int E, int64_t rows, int n_per_batch,
                                                               int64_t bstride, int D, int G,
                                                               const float* __restrict__ W,
                                                               double* __restrict__ partial,
                                                               unsigned short* __restrict__ wt) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= E * G) {
    // wt[e][split][j][k] = split of W[e][k][j]: a thread takes 8 consecutive k of one column j
    const int64_t per_tap = (int64_t)(D / 8) * D;
    const int64_t total = per_tap * E;
    const int64_t nthreads = (int64_t)(gridDim.x - E * G) * 256;
    for (int64_t idx = (int64_t)(blockIdx.x - E * G) * 256 + tid; idx < total; idx += nthreads) {
      const int e = (int)(idx / per_tap);
      const int64_t rem = idx - (int64_t)e * per_tap;
      const int j = (int)(rem % D), k0 = (int)(rem / D) * 8;
      const float* src = W + ((size_t)e * D + k0) * D + j;
      float h[8], m[8], l[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float w = src[(size_t)i * D];
        h[i] = bf16_bits_to_f32(f32_to_bf16_bits(w));
        const float r1 = w - h[i];
        m[i] = bf16_bits_to_f32(f32_to_bf16_bits(r1));
        l[i] = r1 - m[i];
      }
      unsigned short* dst = wt + (size_t)e * 3 * D * D + (size_t)j * D + k0;
      const size_t sp = (size_t)D * D;
      *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16_bits(h[0], h[1]), pack_bf16_bits(h[2], h[3]),
                                                  pack_bf16_bits(h[4], h[5]), pack_bf16_bits(h[6], h[7]));
      *reinterpret_cast<uint4*>(dst + sp) = make_uint4(pack_bf16_bits(m[0], m[1]), pack_bf16_bits(m[2], m[3]),
                                                       pack_bf16_bits(m[4], m[5]), pack_bf16_bits(m[6], m[7]));
      *reinterpret_cast<uint4*>(dst + 2 * sp) = make_uint4(pack_bf16_bits(l[0], l[1]), pack_bf16_bits(l[2], l[3]),
                                                           pack_bf16_bits(l[4], l[5]), pack_bf16_bits(l[6], l[7]));
    }
    return;
  }
  __shared__ double red[2048];                 // [row lane][D]: row lanes * D <= 256 * 8
  const int e = blockIdx.x / G, g = blockIdx.x - e * G;
  const int cv = D / 8;                        // 16-byte column vectors per row
  const int nrl = 256 / cv;                    // row lanes
  const int c = tid % cv, rl = tid / cv;
  const int64_t slab = (rows + G - 1) / G;
  const int64_t r_begin = (int64_t)g * slab;
  const int64_t r_end = r_begin + slab < rows ? r_begin + slab : rows;
  const unsigned short* s = tp.s[e];
  double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (rl < nrl) {
    for (int64_t r = r_begin + rl; r < r_end; r += nrl) {
      const int64_t b = r / n_per_batch;
      const uint4 v = *reinterpret_cast<const uint4*>(s + b * bstride + (r - b * n_per_batch) * D + 8 * c);
      float f[8];
      unpack8(v, f);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += (double)f[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[rl * D + 8 * c + i] = acc[i];
  }
  __syncthreads();
  for (int col = tid; col < D; col += 256) {
    double t = 0.0;
    for (int q = 0; q < nrl; ++q) t += red[q * D + col];
    partial[((size_t)e * G + g) * D + col] = t;
  }
}

// launch 2
__global__ __launch_bounds__(256) void selector_token_grad_kernel(TapPtrs tp, int E, int64_t rows, int n_per_batch,
                                                                  int64_t bstride, int D, int G,
                                                                  const float* __restrict__ W,
                                                                  const double* __restrict__ partial,
                                                                  const unsigned short* __restrict__ wt,
                                                                  int64_t ntiles, int panels) {
  extern __shared__ __align__(16) unsigned char smem[];       // [2][3][TG_COLS][TG_PROW] bytes: staged W chunks
  __shared__ float s_mean[TG_MAX_D];
  __shared__ __align__(16) float s_row[TG_MAX_D];
  unsigned char* Pl = smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t total = (int64_t)E * ntiles * panels;
  const int64_t item_begin = total * blockIdx.x / gridDim.x;
  const int64_t item_end = total * (blockIdx.x + 1) / gridDim.x;
  const size_t split_stride = (size_t)D * D;
  int cur_tap = -1;

  for (int64_t item = item_begin; item < item_end; ++item) {
    const int panel = (int)(item % panels);
    const int64_t t2 = item / panels;
    const int64_t tile = t2 % ntiles;
    const int tap = (int)(t2 / ntiles);
    if (tap != cur_tap) {
      // mean of the tap's columns and row = -mean W (subtracted after the product, as s W - mean W)
      // (every workgroup forms them itself, in a fixed order: wave w takes a quarter of the partials / of k, a lane
      // the columns lane, lane + 64, ..., so that the loads of a quarter are independent and in flight together)
      __syncthreads();
      double* red = reinterpret_cast<double*>(smem);            // [4][D] fp64, in front of the first W chunk
      for (int col = lane; col < D; col += 64) {
        double t = 0.0;
        const double* p = partial + (size_t)tap * G * D + col;
#pragma unroll 8
        for (int g = wave; g < G; g += 4) t += p[(size_t)g * D];
        red[wave * D + col] = t;
      }
      __syncthreads();
      for (int col = tid; col < D; col += 256)
        s_mean[col] = (float)((red[col] + red[D + col] + red[2 * D + col] + red[3 * D + col]) / (double)rows);
      __syncthreads();
      const int kq = D / 4;
      for (int col = lane; col < D; col += 64) {
        const float* w = W + ((size_t)tap * D + wave * kq) * D + col;
        double t = 0.0;
#pragma unroll 16
        for (int k = 0; k < kq; ++k) t += (double)s_mean[wave * kq + k] * (double)w[(size_t)k * D];
        red[wave * D + col] = t;
      }
      __syncthreads();
      for (int col = tid; col < D; col += 256)
        s_row[col] = (float)(-(red[col] + red[D + col] + red[2 * D + col] + red[3 * D + col]));
      __syncthreads();
      cur_tap = tap;
    }
    const unsigned short* s = tp.s[tap];
    const unsigned short* wtap = wt + (size_t)tap * 3 * split_stride + (size_t)panel * TG_COLS * D;
    const int64_t r0 = tile * TG_ROWS + wave * 64;

    f32x4 acc[4][TG_NCT];
#pragma unroll
    for (int c = 0; c < TG_NCT; ++c) {
      const f32x4 rv = *reinterpret_cast<const f32x4*>(&s_row[panel * TG_COLS + 16 * c + 4 * (lane >> 4)]);
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g][c] = rv;
    }
    unsigned int xs[4];                          // element offsets of the lane's four token rows (< 2^31: host check)
    bool valid[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t r = r0 + 16 * g + (lane & 15);
      valid[g] = r < rows;
      const int64_t rr = valid[g] ? r : 0;
      const int64_t b = rr / n_per_batch;
      xs[g] = (unsigned int)(b * bstride + (rr - b * n_per_batch) * D + 8 * (lane >> 4));
    }
    // software pipeline over the K chunks as in token_gram_bf16x3_kernel: the loads of chunk c + 1 are issued before
    // the MFMAs of chunk c and land in the other LDS buffer behind them; one barrier per chunk
    constexpr int PVEC = 3 * TG_COLS * 4 / 256;                 // 9 uint4 per thread per chunk
    u32x4 pre[PVEC];
    bf16x8 an[4];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int v = 0; v < PVEC; ++v) {
        const int el = tid + 256 * v;
        const int q = el & 3, rc = el >> 2;
        const int sp = rc / TG_COLS, col = rc - sp * TG_COLS;
        pre[v] = *reinterpret_cast<const u32x4*>(wtap + sp * split_stride + (size_t)col * D + k0 + 8 * q);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        an[g] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        if (valid[g]) an[g] = *reinterpret_cast<const bf16x8*>(s + xs[g] + k0);
      }
    };
    auto stash = [&](unsigned char* buf) {
#pragma unroll
      for (int v = 0; v < PVEC; ++v) {
        const int el = tid + 256 * v;
        const int q = el & 3, rc = el >> 2;
        *reinterpret_cast<u32x4*>(buf + (size_t)rc * TG_PROW + 16 * q) = pre[v];
      }
    };
    __syncthreads();                            // the previous tile's fragment reads are done
    fetch(0);
    stash(Pl);
    bf16x8 a[4] = {an[0], an[1], an[2], an[3]};
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < D; k0 += TG_KC) {
      const bool more = k0 + TG_KC < D;
      if (more) fetch(k0 + TG_KC);
      const unsigned char* Pc = Pl + cur * TG_PBUF;
#pragma unroll
      for (int sp = 0; sp < 3; ++sp) {
#pragma unroll
        for (int c = 0; c < TG_NCT; ++c) {
          const bf16x8 w8 = *reinterpret_cast<const bf16x8*>(
              Pc + (size_t)(sp * TG_COLS + c * 16 + (lane & 15)) * TG_PROW + 16 * (lane >> 4));
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8, a[g], acc[g][c], 0, 0, 0);
        }
      }
      if (more) {
        stash(Pl + (cur ^ 1) * TG_PBUF);
#pragma unroll
        for (int g = 0; g < 4; ++g) a[g] = an[g];
      }
      cur ^= 1;
      __syncthreads();
    }
    // acc[g][c][i]: token row r0 + 16 g + (lane & 15), output column 16 c + 4 (lane >> 4) + i
    unsigned short* out = tp.out[tap];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (!valid[g]) continue;
      const int64_t r = r0 + 16 * g + (lane & 15);
      unsigned short* o = out + r * D + panel * TG_COLS + 4 * (lane >> 4);
#pragma unroll
      for (int c = 0; c < TG_NCT; ++c)
        *reinterpret_cast<uint2*>(o + 16 * c) =
            make_uint2(pack_bf16(acc[g][c][0], acc[g][c][1]), pack_bf16(acc[g][c][2], acc[g][c][3]));
    }
  }
}

// bf16(float(a) + float(b)) of 8 values: the rounding of torch's bf16 add
__device__ __forceinline__ uint4 add8_bf16(const uint4& a, const uint4& b) {
  float x[8], y[8];
  unpack8(a, x);
  unpack8(b, y);
  return make_uint4(pack_bf16(x[0] + y[0], x[1] + y[1]), pack_bf16(x[2] + y[2], x[3] + y[3]),
                    pack_bf16(x[4] + y[4], x[5] + y[5]), pack_bf16(x[6] + y[6], x[7] + y[7]));
}

__global__ __launch_bounds__(256) void tap_grad_scatter_kernel(const uint4* __restrict__ g_out,
                                                               const uint4* __restrict__ g_a,
                                                               const uint4* __restrict__ g_b, int64_t nvec, int T,
                                                               int offset, int dv, uint4* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t per_batch = (int64_t)T * dv;
  const int n_tok = T - offset;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const int64_t b = v / per_batch;
    const int64_t in_b = v - b * per_batch;
    const int t = (int)(in_b / dv);
    uint4 r = make_uint4(0, 0, 0, 0);
    bool have = false;
    if (t >= offset) {
      const int64_t src = (b * n_tok + (t - offset)) * dv + (in_b - (int64_t)t * dv);
      if (g_a != nullptr) { r = g_a[src]; have = true; }
      if (g_b != nullptr) { r = have ? add8_bf16(r, g_b[src]) : g_b[src]; have = true; }
    }
    if (g_out != nullptr) r = have ? add8_bf16(g_out[v], r) : g_out[v];
    out[v] = r;
  }
}

}  // namespace basd

// widths whose columns tile into panels of TG_COLS and fit the LDS mean / row buffers
static bool selector_token_grad_width_ok(int d_s) { return d_s == 192 || d_s == 384 || d_s == 768; }

extern "C" int64_t basd_selector_token_grad_workspace_bytes(int E, int d_s) {
  if (E < 1 || d_s < 1) return 0;
  return (int64_t)E * basd::TG_MAX_G * d_s * 8 + (int64_t)E * 3 * d_s * d_s * 2;
}

extern "C" int basd_selector_token_grad(const void* const* tokens, int E, int B, int N, int D_s, int64_t batch_stride,
                                        const float* w, void* const* out, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  using namespace basd;
  if (E < 1 || E > TG_MAX_E) return fail(BASD_ERR_SHAPE, "selector_token_grad: E=%d out of 1..%d", E, TG_MAX_E);
  if (!selector_token_grad_width_ok(D_s))
    return fail(BASD_ERR_SHAPE, "selector_token_grad: D_s=%d (192, 384 or 768)", D_s);
  if (B < 1 || N < 1) return fail(BASD_ERR_SHAPE, "selector_token_grad: B=%d N=%d", B, N);
  if (batch_stride % 8 || batch_stride < (int64_t)N * D_s)
    return fail(BASD_ERR_SHAPE, "selector_token_grad: batch stride %lld", (long long)batch_stride);
  if ((int64_t)B * batch_stride >= ((int64_t)1 << 31))       // the kernel keeps 32-bit element offsets into a tap
    return fail(BASD_ERR_SHAPE, "selector_token_grad: B * batch_stride = %lld elements, 2^31 or more",
                (long long)((int64_t)B * batch_stride));
  if (workspace == nullptr || workspace_bytes < basd_selector_token_grad_workspace_bytes(E, D_s))
    return fail(BASD_ERR_WORKSPACE, "selector_token_grad: workspace of %lld bytes", (long long)workspace_bytes);
  if (w == nullptr || ((uintptr_t)workspace & 15)) return fail(BASD_ERR_SHAPE, "selector_token_grad: w / workspace");
  TapPtrs tp;
  for (int i = 0; i < TG_MAX_E; ++i) {
    tp.s[i] = i < E ? (const unsigned short*)tokens[i] : nullptr;
    tp.out[i] = i < E ? (unsigned short*)out[i] : nullptr;
    if (i < E && (tp.s[i] == nullptr || tp.out[i] == nullptr || ((uintptr_t)tp.s[i] & 15) || ((uintptr_t)tp.out[i] & 15)))
      return fail(BASD_ERR_SHAPE, "selector_token_grad: tap %d pointer missing or not 16-byte aligned", i);
  }
  const int64_t rows = (int64_t)B * N;
  const int G = tg_partials(rows);
  double* partial = reinterpret_cast<double*>(workspace);
  unsigned short* wt = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(workspace) +
                                                         (size_t)E * TG_MAX_G * D_s * 8);
  hipStream_t st = (hipStream_t)stream;
  const int64_t split_threads = (int64_t)E * (D_s / 8) * D_s;
  const int split_blocks = (int)((split_threads + 255) / 256 < 256 ? (split_threads + 255) / 256 : 256);
  hipLaunchKernelGGL(tap_colsum_split_kernel, dim3(E * G + split_blocks), dim3(256), 0, st, tp, E, rows, N,
                     batch_stride, D_s, G, w, partial, wt);
  int rc = check_launch("selector_token_grad (column sums, W split)");
  if (rc) return rc;
  const int64_t ntiles = (rows + TG_ROWS - 1) / TG_ROWS;
  const int panels = D_s / TG_COLS;
  const int64_t total = (int64_t)E * ntiles * panels;
  const int grid = (int)(total < 256 ? total : 256);
  allow_full_lds((const void*)selector_token_grad_kernel);
  hipLaunchKernelGGL(selector_token_grad_kernel, dim3(grid), dim3(256), 2 * TG_PBUF, st, tp, E, rows, N, batch_stride,
                     D_s, G, w, (const double*)partial, (const unsigned short*)wt, ntiles, panels);
  return check_launch("selector_token_grad");
}


extern "C" int basd_tap_grad_scatter(const void* g_out, const void* g_a, const void* g_b, int B, int T, int D_s,
                                     int offset, void* out, void* stream) {
  using namespace basd;
  if (B < 1 || T < 1 || offset < 0 || offset >= T) return fail(BASD_ERR_SHAPE, "tap_grad_scatter: B=%d T=%d offset=%d", B, T, offset);
  if (D_s < 64 || D_s % 64) return fail(BASD_ERR_SHAPE, "tap_grad_scatter: D_s=%d not a multiple of 64", D_s);
  if (out == nullptr) return fail(BASD_ERR_SHAPE, "tap_grad_scatter: no output");
  if (((uintptr_t)g_out | (uintptr_t)g_a | (uintptr_t)g_b | (uintptr_t)out) & 15)
    return fail(BASD_ERR_SHAPE, "tap_grad_scatter: pointers must be 16-byte aligned");
  const int dv = D_s / 8;
  const int64_t nvec = (int64_t)B * T * dv;
  int64_t grid = (nvec + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(tap_grad_scatter_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)g_out,
                     (const uint4*)g_a, (const uint4*)g_b, nvec, T, offset, dv, (uint4*)out);
  return check_launch("tap_grad_scatter");
}
