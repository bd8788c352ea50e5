// RandomChoice([MixUp, CutMix]) of one batch and its soft targets in ONE launch (training/mixup.py; reference
// src/training/trainer.py:89-92,138 runs torchvision v2).  The partner of sample i is sample (i - 1) mod B; the rolled
// batch is never materialised:
//   MixUp    out[i] = lerp(x[i-1], x[i], lam)      torch's two-branch formula in fp32, bf16 rounded once
//   CutMix   out[i] = x[i-1] inside the box (every channel), x[i] elsewhere: bit copies, each pixel written once
//   targets  out_targets[i, c] = lerp(onehot(y[i-1])[c], onehot(y[i])[c], lam), every element written
// The image part walks the FLAT [B * C * H * W] array in 16-byte vectors (4 fp32 / 8 bf16), grid-stride, <= 2048
// workgroups: a vector's own source and its destination are aligned whenever the base pointers are; the partner
// lies C * H * W elements earlier, so it is a 16-byte load when that count is a multiple of the vector and element
// loads otherwise.  A CutMix vector loads only the source(s) its pixels come from (one read + one write per pixel away
// from the box edge).  The at most VEC - 1 elements behind the last whole vector are done one by one, and pointers that
// are not 16-byte aligned take the same kernel with one-element vectors.  The target rows are written by extra
// workgroups behind the image grid.  Contraction is left to the compiler as in torch's lerp kernel: the blend differs
// from it by at most the rounding of one product.
#include "basd_common.h"

namespace basd {
namespace {

constexpr int MX_THREADS = 256;
constexpr int MX_MAX_BLOCKS = 2048;
constexpr int MX_TGT_BLOCKS = 256;

struct MixArgs {
  int64_t total;        // B * n
  int64_t n;            // C * H * W elements of one sample
  int H, W, HW;
  int mode;             // 0 MixUp, 1 CutMix
  float lam;
  int y0, y1, x0, x1;
  int big;              // total >= 2^32: 64-bit index arithmetic for the pixel position
  int partner_vec;      // n % VEC == 0: the partner of a vector is one aligned vector
};

__device__ __forceinline__ float lerp_f32(float a, float b, float w) {     // at::native::lerp
  const float d = b - a;
  return fabsf(w) < 0.5f ? a + w * d : b - d * (1.0f - w);
}

__device__ __forceinline__ float px_to_f32(unsigned int u) { return __uint_as_float(u); }
__device__ __forceinline__ float px_to_f32(unsigned short u) { return bf16_bits_to_f32(u); }
__device__ __forceinline__ void px_from_f32(float f, unsigned int& u) { u = __float_as_uint(f); }
__device__ __forceinline__ void px_from_f32(float f, unsigned short& u) {  // round to nearest even; NaN -> 0x7fc0
  const unsigned int b = __float_as_uint(f);
  u = f != f ? (unsigned short)0x7fc0 : (unsigned short)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}

template <typename U, int V>
__device__ __forceinline__ void load_px(const U* __restrict__ p, U (&v)[V]) {
  if constexpr (V == 1) {
    v[0] = *p;
  } else {
    static_assert(V * sizeof(U) == 16, "one 16-byte vector");
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    __builtin_memcpy(v, &t, 16);
  }
}

template <typename U, int V>
__device__ __forceinline__ void store_px(U* __restrict__ p, const U (&v)[V]) {
  if constexpr (V == 1) {
    *p = v[0];
  } else {
    uint4 t;
    __builtin_memcpy(&t, v, 16);
    *reinterpret_cast<uint4*>(p) = t;
  }
}

__device__ __forceinline__ int64_t partner_of(const MixArgs& a, int64_t f) {   // same element of sample (i - 1) mod B
  return f >= a.n ? f - a.n : f + (a.total - a.n);
}

// V consecutive elements from flat index f (f + V <= total; f a multiple of V when V > 1)
template <typename U, int V>
__device__ __forceinline__ void mix_elems(const MixArgs& a, const U* __restrict__ x, U* __restrict__ out, int64_t f,
                                          bool partner_vec) {
  constexpr unsigned ALL = (1u << V) - 1u;
  unsigned inbox = 0;                               // bit q: element f + q comes from the partner (CutMix)
  if (a.mode == 1 && a.y1 > a.y0 && a.x1 > a.x0) {
    const unsigned r = a.big ? (unsigned)(f % (int64_t)a.HW) : (unsigned)f % (unsigned)a.HW;   // n = C HW: channel-free
    int y = (int)(r / (unsigned)a.W), xx = (int)(r - (unsigned)y * (unsigned)a.W);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      inbox |= (unsigned)(y >= a.y0 && y < a.y1 && xx >= a.x0 && xx < a.x1) << q;
      if (++xx == a.W) {
        xx = 0;
        if (++y == a.H) y = 0;
      }
    }
  }
  const bool blend = a.mode == 0;
  U own[V], prev[V], res[V];
#pragma unroll
  for (int q = 0; q < V; ++q) own[q] = prev[q] = 0;
  if (blend || inbox != ALL) load_px<U, V>(x + f, own);
  if (blend || inbox != 0) {
    if (partner_vec) {
      load_px<U, V>(x + partner_of(a, f), prev);
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (blend || ((inbox >> q) & 1u)) prev[q] = x[partner_of(a, f + q)];
    }
  }
#pragma unroll
  for (int q = 0; q < V; ++q) {
    if (blend) px_from_f32(lerp_f32(px_to_f32(prev[q]), px_to_f32(own[q]), a.lam), res[q]);
    else res[q] = ((inbox >> q) & 1u) ? prev[q] : own[q];
  }
  store_px<U, V>(out + f, res);
}

// workgroups [0, img_blocks): the images; [img_blocks, gridDim.x): the target rows
template <typename U, int VEC>
__global__ void __launch_bounds__(MX_THREADS) mixup_cutmix_kernel(MixArgs a, const U* __restrict__ x, U* __restrict__ out,
                                                                  int img_blocks, const int64_t* __restrict__ labels,
                                                                  int B, int K, float* __restrict__ tgt, int tgt_vec) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < img_blocks) {
    const int64_t nvec = a.total / VEC;
    const bool pv = VEC == 1 || a.partner_vec != 0;
    for (int64_t v = (int64_t)blockIdx.x * MX_THREADS + tid; v < nvec; v += (int64_t)img_blocks * MX_THREADS)
      mix_elems<U, VEC>(a, x, out, v * VEC, pv);
    if constexpr (VEC > 1) {
      const int64_t f = nvec * VEC + tid;           // fewer than VEC elements are left
      if (blockIdx.x == 0 && f < a.total) mix_elems<U, 1>(a, x, out, f, true);
    }
    return;
  }
  const int tgt_blocks = (int)gridDim.x - img_blocks;
  const float w_own = lerp_f32(0.0f, 1.0f, a.lam), w_prev = lerp_f32(1.0f, 0.0f, a.lam), w_both = lerp_f32(1.0f, 1.0f, a.lam);
  for (int i = (int)blockIdx.x - img_blocks; i < B; i += tgt_blocks) {
    const int64_t yi = labels[i], yp = labels[i == 0 ? B - 1 : i - 1];     // a label outside [0, K) matches no column
    float* row = tgt + (int64_t)i * K;
#define MX_VALUE(c) ((c) == yi ? ((c) == yp ? w_both : w_own) : ((c) == yp ? w_prev : 0.0f))
    if (tgt_vec) {                                   // K % 4 == 0 and tgt 16-byte aligned
      for (int c = 4 * tid; c < K; c += 4 * MX_THREADS)
        *reinterpret_cast<float4*>(row + c) = make_float4(MX_VALUE(c), MX_VALUE(c + 1), MX_VALUE(c + 2), MX_VALUE(c + 3));
    } else {
      for (int c = tid; c < K; c += MX_THREADS) row[c] = MX_VALUE(c);
    }
#undef MX_VALUE
  }
}

template <typename U, int VEC>
void launch_mixup(const MixArgs& args, const void* x, void* out, const int64_t* labels, int B, int K, float* tgt,
                  hipStream_t st) {
  MixArgs a = args;
  a.partner_vec = (a.n % VEC) == 0;
  const int64_t nvec = a.total / VEC;
  int64_t img_blocks = (nvec + MX_THREADS - 1) / MX_THREADS;
  if (img_blocks > MX_MAX_BLOCKS) img_blocks = MX_MAX_BLOCKS;
  if (img_blocks < 1) img_blocks = 1;                // the element tail alone
  const int tgt_blocks = B < MX_TGT_BLOCKS ? B : MX_TGT_BLOCKS;
  const int tgt_vec = K % 4 == 0 && ((uintptr_t)tgt & 15) == 0;
  hipLaunchKernelGGL((mixup_cutmix_kernel<U, VEC>), dim3((unsigned)(img_blocks + tgt_blocks)), dim3(MX_THREADS), 0, st, a,
                     (const U*)x, (U*)out, (int)img_blocks, labels, B, K, tgt, tgt_vec);
}

}  // namespace
}  // namespace basd

extern "C" int basd_mixup_cutmix(const void* images, int img_bf16, int B, int C_img, int H, int W, const int64_t* labels,
                                 int num_classes, int mode, float lam, int y0, int y1, int x0, int x1, void* out_images,
                                 float* out_targets, void* stream) {
  using namespace basd;
  if (B < 1 || num_classes < 1 || C_img < 1 || H < 1 || W < 1)
    return fail(BASD_ERR_SHAPE, "mixup_cutmix: B = %d, num_classes = %d, image %d x %d x %d", B, num_classes, C_img, H, W);
  if (mode != 0 && mode != 1) return fail(BASD_ERR_SHAPE, "mixup_cutmix: mode %d (0 MixUp, 1 CutMix)", mode);
  if (mode == 1 && (y0 < 0 || y0 > y1 || y1 > H || x0 < 0 || x0 > x1 || x1 > W))
    return fail(BASD_ERR_SHAPE, "mixup_cutmix: box [%d, %d) x [%d, %d) outside %d x %d", y0, y1, x0, x1, H, W);
  if (images == nullptr || labels == nullptr || out_images == nullptr || out_targets == nullptr)
    return fail(BASD_ERR_SHAPE, "mixup_cutmix: null pointer");
  const int64_t n = (int64_t)C_img * H * W;
  if (n > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "mixup_cutmix: %lld elements per sample", (long long)n);
  const int64_t total = (int64_t)B * n;
  const size_t esize = img_bf16 ? 2 : 4;
  const uintptr_t src = (uintptr_t)images, dst = (uintptr_t)out_images, bytes = (uintptr_t)total * esize;
  if (src < dst + bytes && dst < src + bytes)      // the partner row would be read after it was written
    return fail(BASD_ERR_SHAPE, "mixup_cutmix: out_images overlaps images");
  if (((src | dst) & (esize - 1)) != 0 || ((uintptr_t)out_targets & 3) != 0 || ((uintptr_t)labels & 7) != 0)
    return fail(BASD_ERR_SHAPE, "mixup_cutmix: a pointer is not aligned to its element");
  MixArgs a;
  a.total = total;
  a.n = n;
  a.H = H;
  a.W = W;
  a.HW = H * W;
  a.mode = mode;
  a.lam = lam;
  a.y0 = y0; a.y1 = y1; a.x0 = x0; a.x1 = x1;
  a.big = total > 0xffffffffLL;
  a.partner_vec = 0;
  const bool wide = ((src | dst) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (img_bf16) {
    if (wide) launch_mixup<unsigned short, 8>(a, images, out_images, labels, B, num_classes, out_targets, st);
    else launch_mixup<unsigned short, 1>(a, images, out_images, labels, B, num_classes, out_targets, st);
  } else {
    if (wide) launch_mixup<unsigned int, 4>(a, images, out_images, labels, B, num_classes, out_targets, st);
    else launch_mixup<unsigned int, 1>(a, images, out_images, labels, B, num_classes, out_targets, st);
  }
  return check_launch("mixup_cutmix");
}
