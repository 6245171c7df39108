// conv3 data gradient of the fp32-accurate ("split") learner, image-resident:
// dX2[9][9][64] = (sum over the 3x3 taps of dY3 * w3) * (y2 > 0) with dY3 = hi + lo and
// w3 = hi + lo bf16 planes (backward of duelling_network.py:12-13, learner.py:56), per
// image an 81 x 64 x 576 GEMM of three bf16 products per term.
//
// The generic implicit GEMM (csrc/conv_mfma.hip igemm_dma_kernel<1, true, true, 9, 81,
// true, 2, 64>) runs it as 64-row tiles that each stage the whole hi + lo weight matrix
// (147 KB) and an im2col copy of their dY3 rows through a 2-stage LDS ring: ~190 MB of
// L2 -> LDS traffic for 6.4 MB of dY3 at 512 images.  Here a persistent workgroup (8
// waves, one per CU) walks whole images in static strided order, like the bf16 learner's
// conv3_dgrad_img_kernel (csrc/conv2_img.hip):
//   * dY3 hi and lo (7 x 7 x 64 each) sit in LDS inside a 2-pixel zero ring -- the 11 x 11
//     ring geometry of the conv2 data-gradient kernels, at a slot pitch of 9 (C3S_SLOTS
//     below) and with a chunk placement of its own (c3s_dyoff) --, so out-of-range taps
//     read zeros;
//   * wave w owns output channels 16 (w & 3) .. +15 of pixel tiles 3 (w >> 2) .. +2 (six
//     16-pixel tiles cover the 81 pixels; rows past 80 repeat pixel 80 and are never
//     stored) and keeps its hi + lo weight fragments of the full K in registers (9 taps x
//     2 sub-steps x 2 planes x 4 = 144), fetched once per workgroup: the weight's 64 x 64
//     tap tiles pass through LDS as K-major images (swz_tr) and are read back with the
//     transpose read (tr_frag8), six tap tiles per round in the space that afterwards
//     holds the images;
//   * the results go through LDS and leave as coalesced 16-byte rows of the hi and lo
//     planes with the y2 mask applied to both;
//   * both LDS images are double-buffered, so an image costs ONE barrier: the next image's
//     dY3 and this image's mask are loaded under the MFMA chain, the dY3 goes into the other
//     buffer right after the chain, and the copy-out of image i may still run in some waves
//     while others are in the chain of image i + 1.  All global loads and their waits are
//     unconditional (clamped indices, duplicate lanes): gfx950 counts loads and stores in
//     one vmcnt, and a wait the compiler has to place conservatively (a load under a
//     branch) lands right behind the previous image's stores and exposes their round trip.
//
// The arithmetic is the generic kernel's, so both output planes are the same bits:
// v_mfma_f32_16x16x32_bf16 with the weights as the first operand, one fp32 accumulator
// chain per output from zero over K tile t = 0 .. 8 (dY3 pixel (oh - 2 + t / 3, ow - 2 +
// t % 3), weight tap 8 - t) and its two 32-channel sub-steps, per sub-step the products
// (w_lo, dY_hi), (w_hi, dY_lo), (w_hi, dY_hi); then acc * 1 + 0 (the generic epilogue's
// scale and bias: a -0 sum becomes +0), split_pk_bf16 and mask_bf16x2 of both planes.
#include <type_traits>
#include "mfma_common.h"
// (staging registers of the weight prologue: arrays of HIP's uint4 struct stayed in scratch
// there, 208 B per lane; the native vector type is promoted to registers)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Conv3DgradSplitDesc {
  const bf16_t* dy;     // [N][7][7][64] hi plane
  const bf16_t* dy_lo;
  const bf16_t* w;      // [64 co][3][3][64 ci] OHWI hi plane
  const bf16_t* w_lo;
  const bf16_t* mask;   // y2 hi plane [N][9][9][64] (ReLU mask source)
  bf16_t* dx;           // [N][9][9][64] hi plane
  bf16_t* dx_lo;
  int N;
  // the problem, checked by the launcher (it covers 7 x 7 x 64 -> 9 x 9 x 64, 3 x 3 / 1)
  int H, W, Cout, Cin, KH, KW, stride;
};

#define C3S_THREADS 512
// dY3 slots: padded pixel (row, col) of the 11 x 11 ring geometry is slot 9 row + col.  The
// pitch is the OUTPUT width, so output pixel p = 9 ih + iw reads tap (kh, kw) at slot
// p + 9 kh + kw: the 16 pixel rows of an MFMA fragment read 16 consecutive slots.  Columns 9
// and 10 of a row fall on columns 0 and 1 of the next: all four are ring zeros (dY3 occupies
// columns 2 .. 8), so the overlap stores nothing twice.
// The image is stored chunk-major: 16-B chunk c (8 channels) of slot `slot` at
// c * C3S_CPL + 16 slot (c3s_dyoff), C3S_CPL a multiple of the 256-B bank row.  A
// ds_read_b128 is served in four groups of 16 lanes that are not consecutive lanes:
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, i.e. eight of a fragment's
// 16 pixel rows with chunk c and the other eight with chunk c + 1.  Here the first eight
// take the bank positions of their slots mod 16 and the other eight those of theirs: 16
// different ones from any first slot (the c2d_off swizzle of pixel-major 128-B slots is
// conflict-free for that only where the first slot is a multiple of 4, and the taps shift
// it; with the conv2 kernels' pitch of 11 a fragment that crosses an output row also wraps
// mod 16).  And the address is linear: one register per pixel tile, the tap, the sub-step
// and the lo plane are instruction offsets -- no address arithmetic inside the MFMA chain.
#define C3S_SLOTS 101                    // 9 * 10 + 10 is the last one
#define C3S_CPL 1792                     // bytes of one chunk plane (112 slots)
#define C3S_DY (8 * C3S_CPL)             // one dY3 precision plane; lo follows hi
#define C3S_BUF (2 * C3S_DY)             // one dY3 buffer
#define C3S_OUT (81 * 128)               // one output plane; lo follows hi
#define C3S_SOUT (2 * C3S_BUF)           // start of the two output buffers
#define C3S_LDS (C3S_SOUT + 4 * C3S_OUT)
#define C3S_WTILE 8192                   // one 64 x 64 weight tap tile
#define C3S_WROUND 6                     // tap tiles per prologue round (18 = 9 taps x 2 planes)
static_assert(C3S_SLOTS * 16 <= C3S_CPL && C3S_CPL % 256 == 0, "chunk plane");
static_assert(C3S_WROUND * C3S_WTILE <= C3S_LDS, "the weight rounds reuse the image space");

// output images: csrc/conv2_img.hip c2d_off, 16-B chunk c of pixel row `slot` at c ^ ((slot >> 1) & 7)
__device__ __forceinline__ int c3s_off(int slot, int c) { return (slot << 7) + ((c ^ ((slot >> 1) & 7)) << 4); }
__device__ __forceinline__ int c3s_dyoff(int slot, int c) { return c * C3S_CPL + (slot << 4); }

__global__ void __launch_bounds__(C3S_THREADS, 1) conv3_dgrad_img_split_kernel(Conv3DgradSplitDesc d) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[C3S_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nt = wv & 3, ph = wv >> 2;
  const int l15 = lane & 15, g = lane >> 4;
  const int G = (int)gridDim.x;
  // Thread t moves chunks t and min(t + 512, last) of the 784 dY3 chunks of an image (hi
  // 0 .. 391, lo 392 .. 783) and of the 648 mask / output chunks: the threads past the end
  // repeat the last chunk (same data to the same place) instead of branching.
  // (Those chunk indices and LDS offsets are recomputed where they are used, from opaque
  // copies of the thread index: kept live across the MFMA chain they cost registers the
  // chain does not have.)
#define C3S_TID(v_) \
  int v_ = tid;     \
  asm volatile("" : "+v"(v_));
#define C3S_DK1(t_) (min((t_) + C3S_THREADS, 783) - 392)
#define C3S_MK1(t_) min((t_) + C3S_THREADS, 647)
  // LDS offsets of thread t_'s two dY3 chunks inside a buffer
#define C3S_DST(t_, d0_, d1_)                                                                      \
  int d0_, d1_;                                                                                    \
  {                                                                                                \
    const int pl_ = (t_) >= 392 ? 1 : 0, kk_ = (t_) - 392 * pl_, px_ = kk_ >> 3, oh_ = px_ / 7;    \
    d0_ = pl_ * C3S_DY + c3s_dyoff((oh_ + 2) * 9 + px_ - oh_ * 7 + 2, kk_ & 7);                    \
    const int k1_ = C3S_DK1(t_), px1_ = k1_ >> 3, oh1_ = px1_ / 7;                                 \
    d1_ = C3S_DY + c3s_dyoff((oh1_ + 2) * 9 + px1_ - oh1_ * 7 + 2, k1_ & 7);                       \
  }
  uint4 dv0, dv1, mv0, mv1;
#define C3S_LOAD_DY(IMG, t_)                                                              \
  {                                                                                       \
    const int64_t o_ = (int64_t)(IMG) * 49 * 8;                                           \
    dv0 = ((t_) < 392 ? reinterpret_cast<const uint4*>(d.dy) + o_                         \
                      : reinterpret_cast<const uint4*>(d.dy_lo) + o_ - 392)[t_];          \
    dv1 = reinterpret_cast<const uint4*>(d.dy_lo)[o_ + C3S_DK1(t_)];                      \
  }
  // dY3 of the first image is in flight while the weights are fetched (the launcher caps
  // the grid to the images: blockIdx.x < N)
  C3S_LOAD_DY(blockIdx.x, tid);
  // weight fragments wh / wl[t][s]: rows ci = 16 nt + (lane & 15), K = co 32 s + 8 (lane >> 4)
  // .. + 7 of weight tap 8 - t.  Thread (co = tid >> 3, chunk = tid & 7) copies its 16 bytes
  // of each tap tile (coalesced 128-B rows of w[co][tap][:]) into the K-major image.
  bf16x8 wh[9][2], wl[9][2];
  {
    const int co = tid >> 3, c = tid & 7;
    // (two named staging sets: the next round's loads fly while this round's fragments are read)
    u32x4 stg0[C3S_WROUND], stg1[C3S_WROUND];
    auto load_w = [&](auto rc, u32x4 (&dst)[C3S_WROUND]) {
      constexpr int r = decltype(rc)::value;
#pragma unroll
      for (int i = 0; i < C3S_WROUND; ++i) {
        const int q = r * C3S_WROUND + i, pl = q >= 9 ? 1 : 0;
        dst[i] = reinterpret_cast<const u32x4*>(pl ? d.w_lo : d.w)[(co * 9 + q - 9 * pl) * 8 + c];
      }
    };
    auto round_w = [&](auto rc, u32x4 (&cur)[C3S_WROUND], u32x4 (&nxt)[C3S_WROUND]) {
      constexpr int r = decltype(rc)::value;
      if (r) __syncthreads();   // the previous round's fragment reads are done
#pragma unroll
      for (int i = 0; i < C3S_WROUND; ++i) *reinterpret_cast<u32x4*>(smem + i * C3S_WTILE + swz_tr(co, c)) = cur[i];
      if constexpr (r + 1 < 18 / C3S_WROUND) load_w(std::integral_constant<int, r + 1>{}, nxt);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < C3S_WROUND; ++i) {
        const int q = r * C3S_WROUND + i, pl = q >= 9 ? 1 : 0, t = 8 - (q - 9 * pl);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 f = tr_frag8(smem + i * C3S_WTILE, s, 16 * nt, lane);
          if (pl) wl[t][s] = f;
          else wh[t][s] = f;
        }
      }
    };
    load_w(std::integral_constant<int, 0>{}, stg0);
    round_w(std::integral_constant<int, 0>{}, stg0, stg1);
    round_w(std::integral_constant<int, 1>{}, stg1, stg0);
    round_w(std::integral_constant<int, 2>{}, stg0, stg1);
  }
  __syncthreads();
  // the zero rings of both dY3 buffers, then the first image into buffer 0
  for (int i = tid; i < C3S_SOUT / 16; i += C3S_THREADS)
    *reinterpret_cast<uint4*>(smem + i * 16) = make_uint4(0, 0, 0, 0);
  __syncthreads();
  {
    C3S_DST(tid, dst0, dst1)
    *reinterpret_cast<uint4*>(smem + dst0) = dv0;
    *reinterpret_cast<uint4*>(smem + dst1) = dv1;
  }
  __syncthreads();
  int buf = 0;
  for (int img = blockIdx.x; img < d.N; img += G, buf ^= 1) {
    // Hazards of the one barrier per image (B_i, before the copy-out): dY3 buffer b is
    // written after the chain of image i - 1 and read by the chain of image i, B_(i-1)
    // between; it is rewritten after the chain of image i + 1, which every wave starts
    // behind B_i, i.e. after all chains of image i.  Output buffer b is written before B_i,
    // read after it, and written again before B_(i+2) by waves that passed B_(i+1), which
    // every wave reaches only after its copy-out of image i.
    {
      C3S_TID(tq)
      const uint4* msrc = reinterpret_cast<const uint4*>(d.mask) + (int64_t)img * 648;
      mv0 = msrc[tq];
      mv1 = msrc[C3S_MK1(tq)];
      C3S_LOAD_DY(min(img + G, d.N - 1), tq);   // (the last image again where no next one exists)
    }
    // this lane's three output pixels = the slots of their dY3 pixel (ih - 2, iw - 2), as the
    // address of chunk g in this image's buffer; tap t adds (t / 3) * 9 + t % 3 slots and
    // sub-step s four chunk planes, both constants.  (From an opaque copy of the lane row,
    // per image: hoisted out of the image loop, the compiler keeps more offsets in
    // registers than it has and spills.)
    int sb[3];
    {
      int lq = l15;
      asm volatile("" : "+v"(lq));
#pragma unroll
      for (int j = 0; j < 3; ++j) sb[j] = c3s_dyoff(min((3 * ph + j) * 16 + lq, 80), g) + buf * C3S_BUF;
    }
    f32x4 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // dY3 fragments (hi, lo of the three pixel tiles) of sub-step u + 1 = (t, s) are read
    // while sub-step u's nine MFMAs run (explicit order: scheduler barriers around each)
    bf16x8 xf[2][3][2];
#define C3S_LDX(u_, dst_)                                                                        \
    {                                                                                            \
      const int t_ = (u_) >> 1, k_ = c3s_dyoff((t_ / 3) * 9 + t_ % 3, 4 * ((u_) & 1));            \
      _Pragma("unroll") for (int j = 0; j < 3; ++j) {                                            \
        const int off_ = sb[j] + k_;                                                             \
        dst_[j][0] = *reinterpret_cast<const bf16x8*>(smem + off_);                              \
        dst_[j][1] = *reinterpret_cast<const bf16x8*>(smem + C3S_DY + off_);                     \
      }                                                                                          \
    }
    C3S_LDX(0, xf[0])
#pragma unroll
    for (int u = 0; u < 18; ++u) {
      const int t = u >> 1, s = u & 1;
      if (u + 1 < 18) C3S_LDX(u + 1, xf[(u + 1) & 1])
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[t][s], xf[u & 1][j][0], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[t][s], xf[u & 1][j][1], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[t][s], xf[u & 1][j][0], acc[j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#undef C3S_LDX
    // the next image's dY3 into the other buffer
    {
      C3S_TID(tq)
      C3S_DST(tq, dst0, dst1)
      uint8_t* nb = smem + (buf ^ 1) * C3S_BUF;
      *reinterpret_cast<uint4*>(nb + dst0) = dv0;
      *reinterpret_cast<uint4*>(nb + dst1) = dv1;
    }
    // D[ci][pixel]: the lane holds pixel l15 of each tile, channels 16 nt + 4 g .. + 3
    uint8_t* const sout = smem + C3S_SOUT + buf * (2 * C3S_OUT);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int pix = (3 * ph + j) * 16 + l15;
      if (pix < 81) {
        const int ch = 16 * nt + 4 * g;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[j][r] * 1.0f + 0.0f;
        uint32_t h01, l01, h23, l23;
        split_pk_bf16(v[0], v[1], h01, l01);
        split_pk_bf16(v[2], v[3], h23, l23);
        const int o = c3s_off(pix, ch >> 3) + (ch & 7) * 2;
        *reinterpret_cast<uint2*>(sout + o) = make_uint2(h01, h23);
        *reinterpret_cast<uint2*>(sout + C3S_OUT + o) = make_uint2(l01, l23);
      }
    }
    __syncthreads();
    // (opaque uses: the waits for both mask loads stand here, outside the branch below)
    asm volatile("" : "+v"(mv0.x), "+v"(mv0.y), "+v"(mv0.z), "+v"(mv0.w));
    asm volatile("" : "+v"(mv1.x), "+v"(mv1.y), "+v"(mv1.z), "+v"(mv1.w));
    uint4* dst = reinterpret_cast<uint4*>(d.dx) + (int64_t)img * 648;
    uint4* dsl = reinterpret_cast<uint4*>(d.dx_lo) + (int64_t)img * 648;
    C3S_TID(tc)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = i ? C3S_MK1(tc) : tc;
      const int o = c3s_off(k >> 3, k & 7);
      uint4 v = *reinterpret_cast<const uint4*>(sout + o);
      uint4 vl = *reinterpret_cast<const uint4*>(sout + C3S_OUT + o);
      const uint4 m = i ? mv1 : mv0;
      v = make_uint4(mask_bf16x2(v.x, m.x), mask_bf16x2(v.y, m.y), mask_bf16x2(v.z, m.z), mask_bf16x2(v.w, m.w));
      vl = make_uint4(mask_bf16x2(vl.x, m.x), mask_bf16x2(vl.y, m.y), mask_bf16x2(vl.z, m.z),
                      mask_bf16x2(vl.w, m.w));
      if (i == 0 || tc < 648 - C3S_THREADS) {
        dst[k] = v;
        dsl[k] = vl;
      }
    }
  }
#undef C3S_LOAD_DY
#undef C3S_DST
#undef C3S_TID
}

// grid: workgroups (0: 256), capped to the images.  An uncovered problem, a missing plane
// or a pointer off a 16-byte boundary is refused (hipErrorInvalidValue) and nothing runs.
APEX_EXPORT int apex_conv3_dgrad_img_split(Conv3DgradSplitDesc d, int grid, hipStream_t st) {
  if (d.N <= 0 || d.H != 7 || d.W != 7 || d.Cout != 64 || d.Cin != 64 || d.KH != 3 || d.KW != 3 || d.stride != 1)
    return (int)hipErrorInvalidValue;
  if (d.dy == nullptr || d.dy_lo == nullptr || d.w == nullptr || d.w_lo == nullptr || d.mask == nullptr ||
      d.dx == nullptr || d.dx_lo == nullptr)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)d.dy | (uintptr_t)d.dy_lo | (uintptr_t)d.w | (uintptr_t)d.w_lo | (uintptr_t)d.mask |
       (uintptr_t)d.dx | (uintptr_t)d.dx_lo) & 15)
    return (int)hipErrorInvalidValue;
  if (grid < 0) return (int)hipErrorInvalidValue;
  int G = grid > 0 ? grid : 256;
  if (G > d.N) G = d.N;
  conv3_dgrad_img_split_kernel<<<G, C3S_THREADS, 0, st>>>(d);
  APEX_CHECK_LAUNCH();
}
