// conv3 weight gradient of the fp32-accurate ("split") learner, image-resident:
// dW3[64 co][3][3][64 ci] = sum over images and output pixels of dY3[pixel][co] *
// y2[pixel + tap][ci], db3[co] = sum of dY3, with dY3 = hi + lo and y2 = hi + lo bf16 planes
// (backward of duelling_network.py:12-13), three bf16 products per term.
//
// The generic implicit GEMM (csrc/igemm_wgrad.h igemm_wgrad_body<1, 7, 49, 1, 3, 1>) stages
// per 64-row step one dY3 tile and three im2col tiles of y2, hi + lo: every y2 pixel passes
// L2 -> LDS nine times (once per tap) and dY3 three times, ~76 MB at 512 images, and one
// wave in four has no tile.  Here a persistent workgroup (8 waves, one per CU) walks a
// contiguous range of images and keeps the whole 64 x 576 gradient in registers:
//   * per image dY3 (7 x 7 x 64) and y2 (9 x 9 x 64), hi + lo, arrive ONCE by LDS-DMA,
//     double-buffered (image i + 1 lands while image i computes), 33 KB per image;
//   * dY3 sits on a 9-wide pixel grid of 64 rows (row 9 oh + ow), so the reduction
//     dimension of an image is exactly two K = 32 MFMA steps and reduction row r meets y2
//     slot r + 9 kh + kw at tap (kh, kw).  The 15 rows that are no output pixel (columns 7, 8
//     of each grid row, row 63) hold zeros, as do y2 slots 81 .. 87 (rows up to 63 + 20 = 83
//     are read): written once per buffer, never touched by a DMA piece (those lanes are
//     masked off), so a zero dY3 row never meets anything but finite y2 or zero;
//   * both operands are pixel-major, channel-contiguous images read with the transposed
//     LDS read (ds_read_b64_tr_b16): 128-B rows with the swz_tr chunk swizzle keyed by the
//     ABSOLUTE row.  A 32-lane half of that read covers rows x .. x + 3 and x + 8 .. x + 11
//     of one 32-B column pair: bits 0, 1 of the row take all four values within a run of
//     four and bit 3 differs between the runs, so the eight rows land on eight different
//     (row parity, swizzled pair) positions = 64 different banks for ANY first row x -- the
//     tap shifts cost no conflicts;
//   * wave w = (32-channel co half w & 1) x (144-column Kc quarter w >> 1) = 2 x 9 MFMA
//     tiles of 16 x 16 (72 accumulator registers); a 16-column tile never straddles a tap.
//     Arithmetic per tile and K step as the generic SP = 1 body: (x, dy_lo), (x_lo, dy),
//     (x, dy); the bias gradient is two extra MFMAs per K step against an all-ones fragment
//     in the waves of Kc quarter 0;
//   * at the end each workgroup writes one slab plane [64][576] and one bias-slab row for
//     the grad_finalize job (nsplit = workgroups).  No atomics, no grid barrier.
// The summation order differs from the generic kernel's (per-image chunks per workgroup
// range instead of 384-row splits): same precision class, not the same bits.
#include "igemm_wgrad.h"

#define C3W_THREADS 512
#define C3W_DY 8192                       // one dY3 plane: 64 rows of 128 B
#define C3W_XROWS 88                      // y2 slots 0 .. 80, zero slots up to 87 (11 DMA pieces)
#define C3W_X (C3W_XROWS * 128)           // one y2 plane
#define C3W_BUF (2 * C3W_DY + 2 * C3W_X)  // dY3 hi, lo, y2 hi, lo
#define C3W_NPIECE (2 * 8 + 2 * 11)       // 1-KB DMA pieces per image
#define C3W_PPW ((C3W_NPIECE + 7) / 8)    // per wave (max)
static_assert(2 * C3W_BUF <= 160 * 1024, "LDS");

// tr_frag8 (csrc/mfma_common.h) from any first row: 8 K rows row0 + 8 (lane >> 4) .. + 7 of
// column col0 + (lane & 15) of a swz_tr image of 128-B rows
__device__ __forceinline__ bf16x8 c3w_frag(const uint8_t* img, int row0, int col0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, pcol = lane & 3;
  const int rA = row0 + 8 * g + q;
  const int cbyte = (col0 + 4 * pcol) * 2;
  const int c16 = cbyte >> 4, within = cbyte & 15;
  const lds_s16x4* pa = (const lds_s16x4*)(img + swz_tr(rA, c16) + within);
  const lds_s16x4* pb = (const lds_s16x4*)(img + swz_tr(rA + 4, c16) + within);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(const_cast<lds_s16x4*>(pa));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(const_cast<lds_s16x4*>(pb));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 v = (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

__global__ void __launch_bounds__(C3W_THREADS, 1) conv3_wgrad_img_kernel(WgradDesc d) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * C3W_BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch = wv & 1, kq = wv >> 1;
  const int b = (int)blockIdx.x, G = (int)gridDim.x;
  // this workgroup's images (the launcher caps the grid to N: at least one each)
  const int i0 = (int)(((int64_t)b * d.N) / G), i1 = (int)(((int64_t)(b + 1) * d.N) / G);

  // zero rows of both buffers (everything: the DMA pieces fill the rest)
  for (int i = tid; i < 2 * C3W_BUF / 16; i += C3W_THREADS)
    *reinterpret_cast<uint4*>(smem + i * 16) = make_uint4(0, 0, 0, 0);

  // ---- DMA pieces: wave w moves pieces p = w + 8 k of an image (0 .. 7 dY3 hi, 8 .. 15 dY3
  // lo, 16 .. 26 y2 hi, 27 .. 37 y2 lo).  A piece fills 8 LDS rows: lane l lands in chunk slot
  // l & 7 of row 8 (piece) + (l >> 3), so it fetches the chunk that swz_tr stores there; lanes
  // of zero rows stay out (voff = ~0).
  uint32_t voff[C3W_PPW];
#pragma unroll
  for (int k = 0; k < C3W_PPW; ++k) {
    const int p = wv + 8 * k;
    const bool isx = p >= 16;
    const int lp = isx ? (p - 16) % 11 : (p & 7);
    const int R = lp * 8 + (lane >> 3);
    const int s = ((R >> 1) & 1) | (((R >> 3) & 1) << 1);
    const int c = (lane & 7) ^ (s << 1);
    const int oh = R / 9, ow = R - 9 * oh;
    const bool ok = isx ? R < 81 : (oh < 7 && ow < 7);
    const int pix = isx ? R : oh * 7 + ow;
    voff[k] = ok && p < C3W_NPIECE ? (uint32_t)(pix * 128 + c * 16) : 0xffffffffu;
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  auto issue_dma = [&](int img, int buf) {
#pragma unroll
    for (int k = 0; k < C3W_PPW; ++k) {
      const int p = wv + 8 * k;
      if (p < C3W_NPIECE) {
        const bool isx = p >= 16;
        const bool lo = isx ? p >= 27 : p >= 8;
        const int lp = isx ? (p - 16) % 11 : (p & 7);
        const uint8_t* src = isx ? reinterpret_cast<const uint8_t*>(lo ? d.x_lo : d.x) + (int64_t)img * (81 * 128)
                                 : reinterpret_cast<const uint8_t*>(lo ? d.dy_lo : d.dy) + (int64_t)img * (49 * 128);
        const uint32_t dst = __builtin_amdgcn_readfirstlane(
            lds0 + (uint32_t)(buf * C3W_BUF + (isx ? 2 * C3W_DY + (lo ? C3W_X : 0) : (lo ? C3W_DY : 0)) + lp * 1024));
        if (voff[k] != 0xffffffffu) dma16_s(src, voff[k], dst);
      }
    }
  };

  // acc[i][j] = D[kc][co]: lane holds kc 144 kq + 16 j + 4 g + {0..3} of co 32 ch + 16 i + (lane & 15)
  // The bias sums leave their MFMA chain every 4 images (196 terms, about a generic split)
  // for a second accumulator: one fp32 chain over a long image range (3,626 terms for 74
  // images in one workgroup) carried 4-5x the generic kernel's db error.
  f32x4 acc[2][9], accb[2], accb_sum[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    accb_sum[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u));
  const bool do_bias = d.bias_slab != nullptr && kq == 0;

  __syncthreads();                        // the zeros are in place before any DMA piece lands
  if (i0 < i1) issue_dma(i0, 0);
  // One barrier per image (B_i): every wave waits for its own pieces of image i, then the
  // barrier makes all of them visible; it also closes every wave's reads of buffer
  // (i + 1) & 1 (image i - 1), which the pieces of image i + 1 issued behind it overwrite.
  // The loop holds no other vector memory operation, so vmcnt(0) counts the pieces alone.
  for (int img = i0, buf = 0; img < i1; ++img, buf ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (img + 1 < i1) issue_dma(img + 1, buf ^ 1);
    const uint8_t* DH = smem + buf * C3W_BUF;
    const uint8_t* DL = DH + C3W_DY;
    const uint8_t* XH = DH + 2 * C3W_DY;
    const uint8_t* XL = XH + C3W_X;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 a[2], al[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = c3w_frag(DH, 32 * kk, 32 * ch + 16 * i, lane);
        al[i] = c3w_frag(DL, 32 * kk, 32 * ch + 16 * i, lane);
      }
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        // Kc column 144 kq + 16 j = tap * 64 + ci0: y2 slot of reduction row r is r + 9 kh + kw
        const int col0 = 144 * kq + 16 * j, tap = col0 >> 6, ci0 = col0 & 63;
        const int kh = tap / 3, toff = 9 * kh + (tap - 3 * kh);
        const bf16x8 x = c3w_frag(XH, 32 * kk + toff, ci0, lane);
        const bf16x8 xl = c3w_frag(XL, 32 * kk + toff, ci0, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, al[i], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, a[i], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, a[i], acc[i][j], 0, 0, 0);
        }
      }
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, al[i], accb[i], 0, 0, 0);
          accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, a[i], accb[i], 0, 0, 0);
        }
      }
    }
    if (do_bias && (((img - i0) & 3) == 3 || img + 1 == i1)) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        accb_sum[i] += accb[i];
        accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
  }

  // ---------------- fp32 partial -> slab[workgroup][co][kc] (float4 along kc), bias_slab[workgroup][co]
  const int g = lane >> 4, pl = lane & 15;
  float* slab = d.slab + (int64_t)b * 64 * 576;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j)
      *reinterpret_cast<f32x4*>(slab + (32 * ch + 16 * i + pl) * 576 + 144 * kq + 16 * j + 4 * g) = acc[i][j];
  if (do_bias && g == 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) d.bias_slab[(int64_t)b * 64 + 32 * ch + 16 * i + pl] = accb_sum[i][0];
  }
}

// 1 when the kernel covers the problem: split-mode conv3 (both lo planes; y2 [N, 9, 9, 64]
// against dY3 [N, 7, 7, 64], 3 x 3 / 1), no fused norm partials (ops/conv.py
// conv3_wgrad_img_covers is the caller's copy of this rule)
static bool conv3_wgrad_img_covers(const WgradDesc& d) {
  return d.mode == 1 && d.H == 9 && d.W == 9 && d.Cin == 64 && d.OH == 7 && d.OW == 7 && d.KH == 3 && d.KW == 3 &&
         d.stride == 1 && d.pad_h == 0 && d.pad_w == 0 && d.Co == 64 && d.Kc == 576 && d.ldd == 64 &&
         d.dy != nullptr && d.x != nullptr && d.dy_lo != nullptr && d.x_lo != nullptr && d.slab != nullptr &&
         d.norm_part == nullptr && d.N > 0 && d.Mred == d.N * 49 &&
         ((((uintptr_t)d.dy | (uintptr_t)d.x | (uintptr_t)d.dy_lo | (uintptr_t)d.x_lo | (uintptr_t)d.slab) & 15) == 0);
}

APEX_EXPORT int apex_slab_reduce(const float* slab, int nsplit, int64_t n, float scale, float* out, const float* bslab,
                                 int nb, float* bout, int s2dC, int Kc, hipStream_t st);

// The contract of apex_conv_wgrad (csrc/conv_mfma.hip) for the covered shape, with nsplit =
// workgroups = slab planes (1 .. N: every workgroup owns at least one image); anything else
// is an error (the caller picks the generic kernel).
APEX_EXPORT int apex_conv3_wgrad_img(WgradDesc d, float* out, float* bout, int nsplit, float scale, hipStream_t st) {
  if (!conv3_wgrad_img_covers(d)) return (int)hipErrorInvalidValue;
  if (nsplit < 1 || nsplit > d.N) return (int)hipErrorInvalidValue;
  conv3_wgrad_img_kernel<<<nsplit, C3W_THREADS, 0, st>>>(d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (out != nullptr)
    return apex_slab_reduce(d.slab, nsplit, (int64_t)64 * 576, scale, out, d.bias_slab, d.bias_slab ? 64 : 0, bout, 0,
                            576, st);
  return 0;
}
