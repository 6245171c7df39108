// conv2 data gradient fused with conv1 weight gradient, image-resident (fp32-class
// "split" mode, C = 4 frames, static image order).
//
// Reference: the conv2 -> conv1 part of loss.backward() (learner.py:56).  The pair of
// kernels this replaces at large batches -- conv2_dgrad_img_split_kernel
// (csrc/conv2_img.hip) and conv1_wgrad_img_kernel<4, true> (csrc/conv1_wgrad.hip) --
// hands dY1 (N x 20 x 20 x 64, hi + lo bf16 planes) over through global memory: 52 MB
// written and 52 MB read back at 512 images, for a tensor nothing else reads (conv1 has
// no data gradient).  Here a persistent workgroup (8 waves, one per CU) walks whole
// images; per image it computes the masked dY1 into LDS and consumes it there for the
// dW1 / db1 partials of its image group.
//
//   * dgrad: wave w owns (stride-parity class w >> 1, channel half w & 1) with its hi /
//     lo weight fragments (128 registers) loaded once; the same fragments, K order
//     (s = 0..15), MFMA order (w_lo dY_hi, w_hi dY_lo, w_hi dY_hi), split_pk_bf16 and
//     mask_bf16x2 as conv2_dgrad_img_split_kernel, so every dY1 value is BIT-IDENTICAL
//     to the planes that kernel writes.  The y1 mask words a lane needs are loaded
//     straight from global memory before the MFMA chain of a pass.
//   * the accumulators go straight into the transposed-read (swz_tr) dY1 image that
//     the weight gradient's ds_read_b64_tr_b16 fragments read; dY1 never reaches
//     global memory (unless the debug planes dx / dx_lo are given: tests).
//   * wgrad: wave w owns co half (w & 1) x K quarter (w >> 1) as in
//     conv1_wgrad_img_kernel; the bias gradient is two MFMAs against an all-ones
//     fragment.  The k-steps take the image's pixels in raster order, 32 per step, the
//     same pixels in the same K positions and the same MFMA order as that kernel, and an
//     image group's partial accumulates over the same images in the same order: dW1 /
//     db1 are bit-identical to the pair's as well.  (The wgrad's sum over pixels could run
//     in any order, dW1 / db1 then being only fp64-bounded; a class-major order was built
//     first and dropped: the rounding difference grows through centered RMSprop and
//     prioritised sampling until a run's results are no longer the pair's.)
//
// An image's 400 dY1 rows (hi + lo) do not fit beside the frame planes, so it runs in
// two passes over the dgrad's class-pixel index r (pixel (2 a + p, 2 b + q), a = r / 10,
// b = r % 10, (p, q) the class parity), split where the classes complete image rows:
//   pass 0: r in [0, 60) of all four classes = image rows 0..11 = raster pixels 0..239,
//           dY1 row = pixel; the wgrad consumes k-steps 0..6 (pixels 0..223);
//   pass 1: r in [60, 100) = pixels 240..399: pixels 240..255 at their own rows, pixel
//           pi >= 256 at row pi - 256 (0..143), rows 144..159 zeroed; k-step 7 reads rows
//           224..255, k-steps 8..12 rows 0..159.  13 k-steps per image.
//
// LDS (159,744 B of 163,840):
//   frame planes, bf16 (frame c, half h: 441 x 16 B)   57,344
//   dY1 image, 256 rows x 128 B x (hi, lo)              65,536
//   dY2 slot images in their zero ring, hi + lo         36,864
// The uint8 staging copy of the NEXT image's frames (28,672 B, LDS-DMA) aliases the dY2
// images, which are dead after pass 1's MFMAs: it lands under the second wgrad half,
// is converted to planes after the end-of-image barrier, and then the next image's dY2
// is copied over it, zero ring included -- from rows 160..255 of the dY1 planes, free
// once k-step 7 has read them, where an LDS-DMA puts it under k-steps 8..12.
#include "mfma_common.h"
#include "conv2_wfrag.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Conv21BwdDesc {
  const bf16_t* dy;         // dY2 [N][9][9][64], hi plane
  const bf16_t* dy_lo;      // lo plane
  const bf16_t* w;          // conv2 weights [64 co][4][4][64 ci] OHWI hi / lo: read only by the
  const bf16_t* w_lo;       //   launcher's pack when !wfrag_ready
  const bf16_t* mask;       // y1 [N][20][20][64] (ReLU mask source, hi plane)
  uint4* wfrag;             // weights in fragment order, hi then lo (csrc/conv2_wfrag.h)
  int wfrag_ready;
  const uint8_t* ring;      // s2d frame ring [F][21][21][16]
  const int32_t* slots;     // [N][4]
  const uint8_t* zero16;    // 16 zero bytes (DMA filler)
  float* slab;              // [grid][64][256] partials (s2d K order)
  float* bias_slab;         // [grid][64]
  bf16_t* dx;               // debug: masked dY1 planes [N][20][20][64] (hi, lo), or both null
  bf16_t* dx_lo;
  unsigned long long* wq;   // must be null: the work queue is not implemented here
  int N, C;
};

#define F21_THREADS 512
#define F21_PLANE 7168                  // one frame half-plane: 441 x 16 B, padded
#define F21_IMG (8 * F21_PLANE)         // 4 frames x 2 halves
#define F21_DYPL (256 * 128)            // one dY1 plane
#define F21_S2PL (144 * 128)            // one dY2 slot image (C2D_PSLOTS of csrc/conv2_img.hip)
#define F21_NCHUNK (4 * 441)            // 16-B chunks of an image's frames
#define F21_NDMA 28                     // 1-KB frame DMA instructions per image
#define F21_NDY2 11                     // 1-KB dY2 DMA instructions per plane (648 chunks)

__device__ __forceinline__ int f21_c2d_off(int slot, int c) { return (slot << 7) + ((c ^ ((slot >> 1) & 7)) << 4); }

__global__ void __launch_bounds__(256) pack_c2d_wfrag21_kernel(const bf16_t* __restrict__ w,
                                                               const bf16_t* __restrict__ w_lo,
                                                               uint32_t* __restrict__ out) {
  pack_c2d_wfrag_word(blockIdx.x * 256 + threadIdx.x, w, w_lo, out);
}

__global__ void __launch_bounds__(F21_THREADS, 1) conv21_bwd_fused_kernel(Conv21BwdDesc d) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[F21_IMG + 2 * F21_DYPL + 2 * F21_S2PL];
  uint8_t* Pl = smem;
  uint8_t* Dy = Pl + F21_IMG;
  uint8_t* S2 = Dy + 2 * F21_DYPL;
  uint8_t* Sg = S2;                     // frame staging aliases the dY2 images
  const int tid = threadIdx.x, lane = tid & 63;
  // (scalar: everything derived from the wave index stays out of the vector registers,
  // which the weight fragments and the two sets of accumulators fill to the brim)
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // dgrad roles
  const int cls = wv >> 1, nh = wv & 1, p = cls >> 1, q = cls & 1;
  const int rr = lane & 31, kg = lane >> 5;
  // wgrad roles
  const int g = lane >> 4, qq = (lane >> 2) & 3, pcol = lane & 3;
  const int wc = wv & 1, wk = wv >> 1;
  const int G = gridDim.x;

  bf16x8 wh[16], wl[16];
  {
    const uint4* __restrict__ wf = d.wfrag + ((cls * 2 + nh) * 16) * 64 + lane;   // pack_c2d_wfrag_word order
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      wh[s] = __builtin_bit_cast(bf16x8, wf[s * 64]);
      wl[s] = __builtin_bit_cast(bf16x8, wf[C2D_FRAGS + s * 64]);
    }
  }
  // X fragment address of this wave's K tiles (tap wk, frame j): lane reads k = 4 pcol .. +3
  int xoff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    xoff[j] = (2 * j + (pcol >> 1)) * F21_PLANE + (((wk >> 1) * 21 + (wk & 1)) << 4) + ((pcol & 1) << 3);

  auto issue_frames = [&](int img) {
    int sl[4];
    sload_slots<4>(d.slots + img * 4, sl);
    int ln = lane;
    asm volatile("" : "+v"(ln));   // (addresses recomputed per image, not held in registers)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = wv * 4 + i;
      if (k < F21_NDMA) {
        const int j = 64 * k + ln;
        const uint8_t* src = d.zero16;
        if (j < F21_NCHUNK) {
          const int c = j / 441, blk = j - c * 441;
          int slot = sl[0];
#pragma unroll
          for (int cc = 1; cc < 4; ++cc)
            if (c == cc) slot = sl[cc];
          src = d.ring + (int64_t)slot * 7056 + (blk << 4);
        }
        const uint32_t off = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)(Sg + k * 1024);
        dma16(src, __builtin_amdgcn_readfirstlane(off));
      }
    }
  };
  auto convert_frames = [&]() {
    for (int j = tid; j < F21_NCHUNK; j += F21_THREADS) {
      const uint4 v = *reinterpret_cast<const uint4*>(Sg + j * 16);
      const int c = j / 441, blk = j - c * 441;
      *reinterpret_cast<uint4*>(Pl + (2 * c) * F21_PLANE + blk * 16) = u8x8_to_bf16x8(v.x, v.y);
      *reinterpret_cast<uint4*>(Pl + (2 * c + 1) * F21_PLANE + blk * 16) = u8x8_to_bf16x8(v.z, v.w);
    }
  };
  // dY2 of one image (hi, lo: 648 chunks each) -> LDS-DMA, as it lies in memory, into rows
  // 160..255 of the dY1 planes, which k-steps 8..12 leave unused ...
  auto issue_dy2 = [&](int img) {
    int ln = lane;
    asm volatile("" : "+v"(ln));   // (addresses recomputed per image, not held in registers)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int k = wv + 8 * i;
      if (k < 2 * F21_NDY2) {
        const int pln = k / F21_NDY2, kk = k - pln * F21_NDY2, j = 64 * kk + ln;
        const uint8_t* src = d.zero16;
        if (j < 81 * 8) src = reinterpret_cast<const uint8_t*>((pln ? d.dy_lo : d.dy) + (int64_t)img * 81 * 64) + j * 16;
        const uint32_t off =
            (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)(Dy + pln * F21_DYPL + 160 * 128 + kk * 1024);
        dma16(src, __builtin_amdgcn_readfirstlane(off));
      }
    }
  };
  // ... -> the slot images, every chunk of both: its pixel's, or zeros in the ring (which
  // the staging copy overwrote)
  auto store_dy2 = [&]() {
    for (int k = tid; k < 2 * 144 * 8; k += F21_THREADS) {
      const int pl = k >= 144 * 8 ? 1 : 0, kk = k - pl * 144 * 8;
      const int slot = kk >> 3, c = (kk & 7) ^ ((slot >> 1) & 7);
      const int row = slot / 11, col = slot - row * 11;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row >= 1 && row <= 9 && col >= 1 && col <= 9)
        v = *reinterpret_cast<const uint4*>(Dy + pl * F21_DYPL + 160 * 128 + (((row - 1) * 9 + col - 1) * 8 + c) * 16);
      *reinterpret_cast<uint4*>(S2 + k * 16) = v;
    }
  };

  f32x4 acc[2][4], accb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u));

  // k-steps [ks0, ks1) of the image (32 raster pixels each, exactly those of
  // conv1_wgrad_img_kernel's k-steps), their dY1 rows starting at row 32 lk0
  auto wg_steps = [&](int ks0, int ks1, int lk0) {
#pragma unroll 1
    for (int ks = ks0; ks < ks1; ++ks) {
      const int p0 = min(32 * ks + 8 * g + qq, 399), p1 = min(32 * ks + 8 * g + qq + 4, 399);
      const int oh0 = p0 / 20, oh1 = p1 / 20;
      const int b0 = ((oh0 * 21 + p0 - 20 * oh0) << 4), b1 = ((oh1 * 21 + p1 - 20 * oh1) << 4);
      const int lk = ks - ks0 + lk0;
      bf16x8 a[2], al[2], b[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = tr_frag8(Dy, lk, 16 * (2 * wc + i), lane);
        al[i] = tr_frag8(Dy + F21_DYPL, lk, 16 * (2 * wc + i), lane);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const lds_s16x4* pa = (const lds_s16x4*)(Pl + b0 + xoff[j]);
        const lds_s16x4* pb = (const lds_s16x4*)(Pl + b1 + xoff[j]);
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(const_cast<lds_s16x4*>(pa));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(const_cast<lds_s16x4*>(pb));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        b[j] = __builtin_bit_cast(bf16x8, (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
      }
      // D[k][co] (swapped operands): lane holds k 16 j + 4 g + {0..3} of co 16 i' + (lane & 15)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], al[i], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
        }
      if (wk == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, al[i], accb[i], 0, 0, 0);
          accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, a[i], accb[i], 0, 0, 0);
        }
      }
    }
  };

  int img = blockIdx.x;
  if (img < d.N) {
    issue_dy2(img);
    issue_frames(img);
  }
  for (; img < d.N; img += G) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's frame DMAs and dY2 DMAs
    __syncthreads();                                   // ... every wave's; the previous image's LDS reads are done
    convert_frames();
    __syncthreads();                                   // staging is read: the dY2 images may replace it
    store_dy2();
    __syncthreads();
    const uint2* __restrict__ mbase = reinterpret_cast<const uint2*>(d.mask + (int64_t)img * 400 * 64);
#pragma unroll
    for (int tp = 0; tp < 2; ++tp) {
      // ---- dgrad pass tp: the two pixel tiles of this wave's class and channel half,
      // one after the other (16 accumulator and 8 mask registers at a time: the weight
      // fragments and the wgrad accumulators leave no room for both tiles at once)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        // (the tile geometry is recomputed from an opaque copy of the lane row, as in
        // conv2_dgrad_img_split_kernel: hoisted, it would hold registers across the image)
        int rq = rr;
        asm volatile("" : "+v"(rq));
        const int rt = (tp == 0 ? 0 : 60) + t * 32 + rq;      // class-pixel index: [0, 60) / [60, 100)
        const bool valid = rt < (tp == 0 ? 60 : 100);
        const int r = min(rt, 99);
        const int pi = r / 10, pj = r - pi * 10;
        const int px = (2 * pi + p) * 20 + 2 * pj + q;         // raster pixel
        const int rho = px < 256 ? px : px - 256;              // its dY1 row
        // y1 words of this lane's 4 channel runs (8 B each): in flight under the MFMAs
        uint2 mv[4];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) mv[g4] = mbase[px * 16 + nh * 8 + 2 * g4 + kg];
        f32x16 dacc;
#pragma unroll
        for (int j = 0; j < 16; ++j) dacc[j] = 0.f;
        // B fragments (dY2 hi, lo) of K step s + 1 are read while step s's MFMAs run
        bf16x8 xf[2][2];
#define F21_LDX(s_, dst_)                                                                    \
        {                                                                                    \
          const int off_ = f21_c2d_off((pi - (((s_) >> 3) & 1) + 1) * 11 + (pj - (((s_) >> 2) & 1) + 1), \
                                       (((s_) & 3) << 1) | kg);                              \
          dst_[0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(S2 + off_)); \
          dst_[1] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(S2 + F21_S2PL + off_)); \
        }
        F21_LDX(0, xf[0])
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          if (s + 1 < 16) F21_LDX(s + 1, xf[(s + 1) & 1])
          __builtin_amdgcn_sched_barrier(0);
          dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[s], xf[s & 1][0], dacc, 0, 0, 0);
          dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s], xf[s & 1][1], dacc, 0, 0, 0);
          dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s], xf[s & 1][0], dacc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
#undef F21_LDX
        // masked hi / lo runs -> row rho of the transposed-read dY1 image
        if (valid) {
          const int sw = (((rho >> 1) & 1) | (((rho >> 3) & 1) << 1)) << 1;
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            uint32_t h01, l01, h23, l23;
            split_pk_bf16(dacc[4 * g4], dacc[4 * g4 + 1], h01, l01);
            split_pk_bf16(dacc[4 * g4 + 2], dacc[4 * g4 + 3], h23, l23);
            const uint2 m = mv[g4];
            const uint2 vh = make_uint2(mask_bf16x2(h01, m.x), mask_bf16x2(h23, m.y));
            const uint2 vl = make_uint2(mask_bf16x2(l01, m.x), mask_bf16x2(l23, m.y));
            const int o = (rho << 7) + (((nh * 4 + g4) ^ sw) << 4) + kg * 8;
            *reinterpret_cast<uint2*>(Dy + o) = vh;
            *reinterpret_cast<uint2*>(Dy + F21_DYPL + o) = vl;
            if (d.dx != nullptr) {
              const int64_t go = ((int64_t)img * 400 + px) * 64 + nh * 32 + 8 * g4 + 4 * kg;
              *reinterpret_cast<uint2*>(d.dx + go) = vh;
              *reinterpret_cast<uint2*>(d.dx_lo + go) = vl;
            }
          }
        }
      }
      if (tp == 1 && tid < 256)   // rows 144..159 of both planes: the last k-step's padding
        *reinterpret_cast<uint4*>(Dy + (tid >> 7) * F21_DYPL + 144 * 128 + (tid & 127) * 16) = make_uint4(0, 0, 0, 0);
      __syncthreads();   // dY1 rows of this pass are complete; dY2 is read (tp == 1: dead)
      if (tp == 0) {
        wg_steps(0, 7, 0);    // pixels 0..223
        __syncthreads();      // pass 1 overwrites rows 0..143
      } else {
        if (img + G < d.N) issue_frames(img + G);   // staging over the dead dY2 images
        wg_steps(7, 8, 7);    // pixels 224..255: rows 224..255
        if (img + G < d.N) {
          __syncthreads();    // rows 160..255 are read
          issue_dy2(img + G);
        }
        wg_steps(8, 13, 0);   // pixels 256..399 and the zero rows: rows 0..159; the DMAs land under these
      }
    }
  }

  // ---- this workgroup's partial: slab[block][co][k] (s2d K order), float4 along k
  float* slab = d.slab + (int64_t)blockIdx.x * 64 * 256;
  const int pl = lane & 15;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = 16 * (2 * wc + i) + pl;
      *reinterpret_cast<f32x4*>(slab + (int64_t)co * 256 + 16 * (4 * wk + j) + 4 * g) = acc[i][j];
    }
  if (wk == 0 && g == 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) d.bias_slab[(int64_t)blockIdx.x * 64 + 16 * (2 * wc + i) + pl] = accb[i][0];
  }
}

APEX_EXPORT int apex_conv21_bwd_fused(Conv21BwdDesc d, int grid, hipStream_t st) {
  if (d.N <= 0 || grid <= 0 || d.C != 4 || d.wq != nullptr) return (int)hipErrorInvalidValue;
  if (d.dy == nullptr || d.dy_lo == nullptr || d.mask == nullptr || d.wfrag == nullptr || d.ring == nullptr ||
      d.slots == nullptr || d.zero16 == nullptr || d.slab == nullptr || d.bias_slab == nullptr)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)d.dy | (uintptr_t)d.dy_lo | (uintptr_t)d.mask | (uintptr_t)d.wfrag | (uintptr_t)d.ring |
       (uintptr_t)d.slots | (uintptr_t)d.zero16 | (uintptr_t)d.slab) & 15)
    return (int)hipErrorInvalidValue;
  if ((uintptr_t)d.bias_slab & 3) return (int)hipErrorInvalidValue;
  if ((d.dx == nullptr) != (d.dx_lo == nullptr) || (((uintptr_t)d.dx | (uintptr_t)d.dx_lo) & 15))
    return (int)hipErrorInvalidValue;
  if (!d.wfrag_ready) {
    if (d.w == nullptr || d.w_lo == nullptr) return (int)hipErrorInvalidValue;
    pack_c2d_wfrag21_kernel<<<C2D_PACK_THREADS / 256, 256, 0, st>>>(d.w, d.w_lo, reinterpret_cast<uint32_t*>(d.wfrag));
  }
  conv21_bwd_fused_kernel<<<grid, F21_THREADS, 0, st>>>(d);
  APEX_CHECK_LAUNCH();
}
