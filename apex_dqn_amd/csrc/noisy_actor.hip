// Per-environment NoisyNet noise for the GPU actor groups (Runtime.noisy_actor_noise = "per_env";
// learner/noisy.py env_noise_vectors is the host mirror and the definition).  Env row e of a batched inference
// call acts under its own draw, and no weight set per env is formed: factorised noise factors through the GEMM,
//
//   W_e x = mu x + xi_out^e * ( sigma (xi_in^e * x) )
//
// so a noisy layer is two products on the shared weights, X mu^T and (X * Xi_in) sigma^T, and an epilogue that
// scales the second per (row, column).  The launches of a call:
//
//   noisy_env_draw_kernel        Xi [E][K] fp32, row e = the concatenated draw at indices e K + k of the counter
//                                word c = 64 u + s (noisy_common.h noisy_xi, the device function of
//                                noisy_compose_kernel: row 0 is the shared draw bit for bit).  u = ctr / every is
//                                read on the device, so a replayed graph draws fresh noise.  One thread per value.
//   noisy_env_fc_kernel          the dual-operand MFMA GEMM of the fc layer over K = 3136 (v_mfma_f32_16x16x32_bf16,
//                                fp32 accumulation).  A block is a tile of 64 env rows x 64 fc columns (one stream:
//                                64 divides 512) over a contiguous run of the 49 K slabs of 64; blockIdx.z is the K
//                                split (noisy_env_ksplit: enough splits that the grid covers the chip at few rows).
//                                The four bf16 weight planes of the slab (wfc hi / lo, swfc hi / lo: the actor
//                                slot's own) are staged once per block into one 32 KiB swizzled LDS image shared by
//                                the four waves; the next slab's global loads are in flight while the current one
//                                is multiplied.  A wave owns 16 rows and reads their X fragments straight from the
//                                hi / lo planes, once, for both products: the gated operand fl32((x_hi + x_lo) xi_in)
//                                is formed in registers from the same fragment and split to hi / lo (bf16 actors:
//                                rounded once), so the two A operands share the X loads and need no LDS.  Two
//                                accumulator sets per tile: P += Whi Xhi + Wlo Xhi + Whi Xlo, S += Shi Ghi + Slo Ghi
//                                + Shi Glo (bf16 actors: the hi planes only).  MFMA operands: A = weights (D row =
//                                fc column), B = activations (D column = env row), so a lane ends with four
//                                consecutive columns of one row: 16-byte stores of both partial planes.
//   noisy_env_fc_epilogue_kernel h = ReLU(P + bfc + Xi_out (S + sbfc)) with P and S the partial planes summed in
//                                increasing split order (no float atomics: two launches are bit-identical), written
//                                as the bf16 planes h (+ h_lo) the head launches read.
//   noisy_env_logits_kernel      the (A + 1) N head logits per env row over K = 512, the same dual-operand scheme
//                                on the fp32 head weights: a block is 64 env rows x 64 head rows of one stream,
//                                mu and sigma are split to bf16 hi + lo on the way into the LDS image (every
//                                element converted once per block), the gated operand is h * Xi_hin, kept as hi +
//                                lo planes in both precisions (the logits are fp32-class functions of the h given,
//                                as the wide heads' are).  MFMA tiles
//                                rather than a wave per (row, head-row group): with fp32 dot products every env row
//                                would stream the 2 J x 512 weights again (J = 1224 at A = 4, N = 255: 5 MB per
//                                row), here a block reads them once for 64 rows.  L [E][Jp] (csrc/wide_head.h's
//                                workspace layout) gets H mu^T + Xi_hout ((H * Xi_hin) sigma^T + sigma_b); mu_b is
//                                added by the finish, which reads it from its head parameters as it does for the
//                                shared path.  The wide actor finish kernels (csrc/qr_wide_head.hip,
//                                csrc/cat_wide_head.hip) turn L into q and the action for N >= 2.
//   noisy_env_scalar_finish_kernel  N = 1: the dueling combine and the epsilon-greedy draw, one thread per env row,
//                                with actor_head_kernel's counter-RNG words (dist_actor_draw).
//
// Nothing depends on the order blocks run in.
#include "noisy_common.h"
#include "wide_head.h"

#define NE_NT 256
#define NE_SLABS (NZ_FC_IN / 64)    // 49 K slabs of the fc layer
#define NE_MAX_KSPLIT 16

struct NoisyEnvDraw {
  float* xi;            // [E][ld]
  int64_t ld;
  int E, A, N, stream;
  uint64_t seed;
  const uint64_t* ctr;
  int64_t every;
};

struct NoisyEnvFc {
  const bf16_t* X; const bf16_t* X_lo;     // [E][3136] (lo: split mode, else null)
  const bf16_t* W; const bf16_t* W_lo;     // wfc planes [1024][3136]
  const bf16_t* S; const bf16_t* S_lo;     // swfc planes
  const float* bfc; const float* sbfc;     // [1024]
  const float* xi;                         // [E][ld]
  int64_t ld;
  int E, ksplit;
  float* part;                             // [ksplit][2][E][1024]
  int64_t n_part;                          // its length (launcher check)
  bf16_t* h; bf16_t* h_lo;                 // [E][1024]
};

struct NoisyEnvLogits {
  const bf16_t* H; const bf16_t* H_lo;     // [E][1024]
  HeadParams mu, sg;
  const float* xi;
  int64_t ld;
  int E, A, N;
  float* L;                                // [E][Jp]
};
static_assert(std::is_standard_layout_v<NoisyEnvDraw> && std::is_trivially_copyable_v<NoisyEnvDraw> &&
              std::is_standard_layout_v<NoisyEnvFc> && std::is_trivially_copyable_v<NoisyEnvFc> &&
              std::is_standard_layout_v<NoisyEnvLogits> && std::is_trivially_copyable_v<NoisyEnvLogits>);

// K splits of the fc GEMM at E rows: row tiles x 16 column tiles x splits >= 256 blocks where 49 slabs allow
static inline int noisy_env_ksplit(int E) {
  const int tiles = ((E + 63) / 64) * (NZ_FC_OUT / 64);
  int ks = (256 + tiles - 1) / tiles;
  return ks < 1 ? 1 : ks > NE_MAX_KSPLIT ? NE_MAX_KSPLIT : ks;
}

// ------------------------------------------------------------------------------------------------ draw
__global__ void __launch_bounds__(NE_NT) noisy_env_draw_kernel(NoisyEnvDraw a) {
  const int K = xi_off(a.A, a.N).K;
  const int64_t i = (int64_t)blockIdx.x * NE_NT + threadIdx.x;
  if (i >= (int64_t)a.E * K) return;
  const int e = (int)(i / K), k = (int)(i - (int64_t)e * K);
  int64_t u = (int64_t)a.ctr[0];
  u = (u < 0 ? 0 : u) / a.every;
  const uint64_t c = (uint64_t)NZ_STREAMS * (uint64_t)u + (uint64_t)a.stream;
  a.xi[(int64_t)e * a.ld + k] = noisy_xi(a.seed, c, (uint32_t)i);
}

// ------------------------------------------------------------------------------------------------ fragments
// 8 activations of one row (bf16 hi, lo or zeros) and their 8 noise values -> the MFMA fragments of the plain and
// of the gated operand g = fl32((hi + lo) xi).  XLO: the activations have a lo plane; GLO: g as hi + lo planes, else
// rounded once to bf16.
struct NeFrag {
  bf16x8 xh, xl, gh, gl;
};
template <bool XLO, bool GLO>
__device__ __forceinline__ NeFrag ne_gate(const uint4& hi, const uint4& lo, const float4& n0, const float4& n1) {
  const uint32_t h[4] = {hi.x, hi.y, hi.z, hi.w}, l[4] = {lo.x, lo.y, lo.z, lo.w};
  const float xi[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
  uint32_t gh[4], gl[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float x0 = __uint_as_float(h[p] << 16), x1 = __uint_as_float(h[p] & 0xffff0000u);
    if (XLO) {
      x0 += __uint_as_float(l[p] << 16);
      x1 += __uint_as_float(l[p] & 0xffff0000u);
    }
    const float g0 = x0 * xi[2 * p], g1 = x1 * xi[2 * p + 1];
    if (GLO) {
      split_pk_bf16(g0, g1, gh[p], gl[p]);
    } else {
      gh[p] = cvt_pk_bf16(g0, g1);
      gl[p] = 0u;
    }
  }
  NeFrag f;
  f.xh = qw_frag(hi);
  f.xl = qw_frag(lo);
  f.gh = qw_frag(make_uint4(gh[0], gh[1], gh[2], gh[3]));
  f.gl = qw_frag(make_uint4(gl[0], gl[1], gl[2], gl[3]));
  return f;
}

// one 32-wide K step of a wave's 16 rows x 64 columns against the LDS image [4][QW_TILE] = (mu hi, mu lo, sigma hi,
// sigma lo): P += Whi Xhi (+ Wlo Xhi with WLO) (+ Whi Xlo with XLO), S += Shi Ghi (+ Slo Ghi with WLO) (+ Shi Glo
// with GLO)
template <bool XLO, bool GLO, bool WLO>
__device__ __forceinline__ void ne_mma(const uint8_t (*Ws)[QW_TILE], int kk, int lane, const NeFrag& f, f32x4* accP,
                                       f32x4* accS) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int off = swz_row(16 * t + (lane & 15), 4 * kk + (lane >> 4));
    const bf16x8 wh = qw_frag(*reinterpret_cast<const uint4*>(&Ws[0][off]));
    const bf16x8 sh = qw_frag(*reinterpret_cast<const uint4*>(&Ws[2][off]));
    accP[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, f.xh, accP[t], 0, 0, 0);
    accS[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sh, f.gh, accS[t], 0, 0, 0);
    if (WLO) {
      const bf16x8 wl = qw_frag(*reinterpret_cast<const uint4*>(&Ws[1][off]));
      const bf16x8 sl = qw_frag(*reinterpret_cast<const uint4*>(&Ws[3][off]));
      accP[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, f.xh, accP[t], 0, 0, 0);
      accS[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sl, f.gh, accS[t], 0, 0, 0);
    }
    if (XLO) accP[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, f.xl, accP[t], 0, 0, 0);
    if (GLO) accS[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sh, f.gl, accS[t], 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------------------ fc
template <bool SPLIT>
__global__ void __launch_bounds__(NE_NT) noisy_env_fc_kernel(NoisyEnvFc a) {
  __shared__ __attribute__((aligned(16))) uint8_t Ws[4][QW_TILE];         // wfc hi, lo, swfc hi, lo: 64 columns x 64 k
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c0 = blockIdx.x * 64;
  const int r = blockIdx.y * 64 + wv * 16 + (lane & 15);
  const int r_ld = min(r, a.E - 1);
  const int z = blockIdx.z;
  const int s_begin = z * NE_SLABS / a.ksplit, s_end = (z + 1) * NE_SLABS / a.ksplit;
  // staging: task = (weight row of the tile, 16-byte chunk of its 64 k), two tasks per thread and plane; job i is
  // task i & 1 of plane i >> 1 = wfc hi, swfc hi, wfc lo, swfc lo (the lo planes in split mode only)
  constexpr int NJ = SPLIT ? 8 : 4;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 wn[NJ];
  const int64_t woff = (int64_t)(c0 + (tid >> 3)) * NZ_FC_IN + 8 * (tid & 7);
  const bf16_t* __restrict__ xsrc = a.X + (int64_t)r_ld * NZ_FC_IN + 8 * (lane >> 4);
  const bf16_t* __restrict__ xsrc_lo = SPLIT ? a.X_lo + (int64_t)r_ld * NZ_FC_IN + 8 * (lane >> 4) : nullptr;
  const float* __restrict__ nsrc = a.xi + (int64_t)r_ld * a.ld + (c0 >= NZ_HID ? NZ_FC_IN : 0) + 8 * (lane >> 4);
  uint4 xh[2], xl[2];
  float4 nz[2][2];
  auto load_slab = [&](int s) {
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      const bf16_t* __restrict__ src = (i >> 1) == 0 ? a.W : (i >> 1) == 1 ? a.S : (i >> 1) == 2 ? a.W_lo : a.S_lo;
      wn[i] = *reinterpret_cast<const u32x4*>(src + woff + (i & 1) * (32 * NZ_FC_IN) + s * 64);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int k = s * 64 + 32 * kk;
      xh[kk] = *reinterpret_cast<const uint4*>(xsrc + k);
      xl[kk] = SPLIT ? *reinterpret_cast<const uint4*>(xsrc_lo + k) : make_uint4(0, 0, 0, 0);
      nz[kk][0] = *reinterpret_cast<const float4*>(nsrc + k);
      nz[kk][1] = *reinterpret_cast<const float4*>(nsrc + k + 4);
    }
  };

  f32x4 accP[4], accS[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) accP[t] = accS[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  load_slab(s_begin);
  for (int s = s_begin; s < s_end; ++s) {
#pragma unroll
    for (int i = 0; i < NJ; ++i)        // planes 0..3 land in Ws[0], [2], [1], [3]
      *reinterpret_cast<u32x4*>(&Ws[((i >> 1) & 1) * 2 + (i >> 2)][swz_row((tid >> 3) + 32 * (i & 1), tid & 7)]) = wn[i];
    NeFrag f[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) f[kk] = ne_gate<SPLIT, SPLIT>(xh[kk], xl[kk], nz[kk][0], nz[kk][1]);
    __syncthreads();
    load_slab(min(s + 1, s_end - 1));   // (the last slab again at the end: no branch around the loads)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) ne_mma<SPLIT, SPLIT, SPLIT>(Ws, kk, lane, f[kk], accP, accS);
    __syncthreads();                    // the image is rewritten at the head of the next slab
  }
  if (r >= a.E) return;
  float* __restrict__ pP = a.part + ((int64_t)(2 * z) * a.E + r) * NZ_FC_OUT + c0 + 4 * (lane >> 4);
  float* __restrict__ pS = pP + (int64_t)a.E * NZ_FC_OUT;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    *reinterpret_cast<float4*>(pP + 16 * t) = make_float4(accP[t][0], accP[t][1], accP[t][2], accP[t][3]);
    *reinterpret_cast<float4*>(pS + 16 * t) = make_float4(accS[t][0], accS[t][1], accS[t][2], accS[t][3]);
  }
}

// h = ReLU(P + bfc + Xi_out (S + sbfc)): one thread per (row, four columns), the partials in increasing split order
__global__ void __launch_bounds__(NE_NT) noisy_env_fc_epilogue_kernel(NoisyEnvFc a) {
  const int e = blockIdx.x, c = 4 * threadIdx.x;
  const int64_t plane = (int64_t)a.E * NZ_FC_OUT;
  const float* __restrict__ p = a.part + (int64_t)e * NZ_FC_OUT + c;
  float4 P = *reinterpret_cast<const float4*>(p), S = *reinterpret_cast<const float4*>(p + plane);
  for (int z = 1; z < a.ksplit; ++z) {
    const float4 u = *reinterpret_cast<const float4*>(p + 2 * z * plane);
    const float4 v = *reinterpret_cast<const float4*>(p + (2 * z + 1) * plane);
    P.x += u.x; P.y += u.y; P.z += u.z; P.w += u.w;
    S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
  }
  const float4 b = *reinterpret_cast<const float4*>(a.bfc + c), sb = *reinterpret_cast<const float4*>(a.sbfc + c);
  const float4 xo = *reinterpret_cast<const float4*>(a.xi + (int64_t)e * a.ld + 2 * NZ_FC_IN + c);
  const float o0 = fmaxf(P.x + b.x + xo.x * (S.x + sb.x), 0.f), o1 = fmaxf(P.y + b.y + xo.y * (S.y + sb.y), 0.f);
  const float o2 = fmaxf(P.z + b.z + xo.z * (S.z + sb.z), 0.f), o3 = fmaxf(P.w + b.w + xo.w * (S.w + sb.w), 0.f);
  const int64_t o = (int64_t)e * NZ_FC_OUT + c;
  if (a.h_lo != nullptr) {
    uint32_t h0, l0, h1, l1;
    split_pk_bf16_h(o0, o1, h0, l0);
    split_pk_bf16_h(o2, o3, h1, l1);
    *reinterpret_cast<uint2*>(a.h + o) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(a.h_lo + o) = make_uint2(l0, l1);
  } else {
    *reinterpret_cast<uint2*>(a.h + o) = make_uint2(pack_bf16x2(o0, o1), pack_bf16x2(o2, o3));
  }
}

// ------------------------------------------------------------------------------------------------ logits
template <bool SPLIT>
__global__ void __launch_bounds__(NE_NT) noisy_env_logits_kernel(NoisyEnvLogits a) {
  __shared__ __attribute__((aligned(16))) uint8_t Ws[4][QW_TILE];         // mu hi, lo, sigma hi, lo: 64 head rows x 64 k
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = a.N, AN = a.A * N, Nv4 = qw_nv4(N), Jp = qr_wide_jp(a.A, N);
  const XiOff xo = xi_off(a.A, N);
  const int r = blockIdx.x * 64 + wv * 16 + (lane & 15);
  const int r_ld = min(r, a.E - 1);
  // the column tile: value tiles first
  const int cv = (N + 63) >> 6;
  const bool val = (int)blockIdx.y < cv;
  const int c0 = ((int)blockIdx.y - (val ? 0 : cv)) * 64;
  const int clim = val ? N : AN;
  // staging: thread = head row tid / 4, 16 consecutive k (two 16-byte chunks of the bf16 row), of mu and of sigma
  const int wr = tid >> 2, seg = tid & 3;
  const int64_t woff = (int64_t)min(c0 + wr, clim - 1) * NZ_HID + seg * 16;
  const float* __restrict__ msrc = (val ? a.mu.wv : a.mu.wa) + woff;
  const float* __restrict__ ssrc = (val ? a.sg.wv : a.sg.wa) + woff;
  const int64_t hoff = (int64_t)r_ld * (2 * NZ_HID) + (val ? 0 : NZ_HID) + 8 * (lane >> 4);
  const bf16_t* __restrict__ hsrc = a.H + hoff;
  const bf16_t* __restrict__ hsrc_lo = SPLIT ? a.H_lo + hoff : nullptr;
  const float* __restrict__ nsrc = a.xi + (int64_t)r_ld * a.ld + (val ? xo.v_in : xo.a_in) + 8 * (lane >> 4);

  float4 mn[4], sn[4];
  uint4 xh[2], xl[2];
  float4 nz[2][2];
  auto load_slab = [&](int s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mn[i] = *reinterpret_cast<const float4*>(msrc + s * 64 + 4 * i);
      sn[i] = *reinterpret_cast<const float4*>(ssrc + s * 64 + 4 * i);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int k = s * 64 + 32 * kk;
      xh[kk] = *reinterpret_cast<const uint4*>(hsrc + k);
      xl[kk] = SPLIT ? *reinterpret_cast<const uint4*>(hsrc_lo + k) : make_uint4(0, 0, 0, 0);
      nz[kk][0] = *reinterpret_cast<const float4*>(nsrc + k);
      nz[kk][1] = *reinterpret_cast<const float4*>(nsrc + k + 4);
    }
  };

  f32x4 accP[4], accS[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) accP[t] = accS[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int NS = NZ_HID / 64;
  load_slab(0);
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      uint4 hi, lo;
      const int off = swz_row(wr, 2 * seg + c);
      qw_split8(mn[2 * c], mn[2 * c + 1], hi, lo);
      *reinterpret_cast<uint4*>(&Ws[0][off]) = hi;
      *reinterpret_cast<uint4*>(&Ws[1][off]) = lo;
      qw_split8(sn[2 * c], sn[2 * c + 1], hi, lo);
      *reinterpret_cast<uint4*>(&Ws[2][off]) = hi;
      *reinterpret_cast<uint4*>(&Ws[3][off]) = lo;
    }
    NeFrag f[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) f[kk] = ne_gate<SPLIT, true>(xh[kk], xl[kk], nz[kk][0], nz[kk][1]);
    __syncthreads();
    if (s + 1 < NS) load_slab(s + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) ne_mma<SPLIT, true, true>(Ws, kk, lane, f[kk], accP, accS);
    __syncthreads();                    // the image is rewritten at the head of the next slab
  }
  if (r >= a.E) return;
  float* __restrict__ Lrow = a.L + (int64_t)r * Jp + (val ? 0 : Nv4);
  const float* __restrict__ xout = a.xi + (int64_t)r * a.ld + (val ? xo.v_out : xo.a_out);
  const float* __restrict__ sb = val ? a.sg.bv : a.sg.ba;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cb = c0 + 16 * t + 4 * (lane >> 4);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (cb + i < clim) Lrow[cb + i] = accP[t][i] + xout[cb + i] * (accS[t][i] + sb[cb + i]);
  }
}

// N = 1: q = v + adv - mean(adv) from L row [v | pad to 4 | adv_0 .. adv_{A-1}] plus the mu biases, then the draw
__global__ void __launch_bounds__(NE_NT) noisy_env_scalar_finish_kernel(ActorIO a, const float* __restrict__ L) {
  const int e = blockIdx.x * NE_NT + threadIdx.x;
  if (e >= a.E) return;
  const int A = a.A;
  const float* __restrict__ row = L + (int64_t)e * qr_wide_jp(A, 1);
  const float v = row[0] + a.P.bv[0];
  float m = 0.f;
  for (int j = 0; j < A; ++j) m += row[4 + j] + a.P.ba[j];
  m /= (float)A;
  int best = 0;
  float bq = -3.4e38f;
  for (int j = 0; j < A; ++j) {
    const float q = v + (row[4 + j] + a.P.ba[j]) - m;
    if (q > bq) { bq = q; best = j; }
    a.q_out[(int64_t)e * A + j] = q;
  }
  dist_actor_draw(best, e, A, a.eps, a.seed, a.ctr, a.a_out);
}

// ------------------------------------------------------------------------------------------------ launchers
static inline bool ne_xi_ok(const float* xi, int64_t ld, int E, int A, int N) {
  if (xi == nullptr || E < 1 || A < 1 || A > HEAD_MAXA || N < 1 || N > 256) return false;
  const int K = xi_off(A, N).K;
  // 16-byte loads of the noise rows; the draw index e K + k as the counter RNG's 32-bit word
  return ld >= K && (ld & 3) == 0 && ((uintptr_t)xi & 15) == 0 && (int64_t)E * K < (1ll << 31);
}

APEX_EXPORT int apex_noisy_env_ksplit(int E) { return noisy_env_ksplit(E < 1 ? 1 : E); }

APEX_EXPORT int apex_noisy_env_draw(NoisyEnvDraw a, hipStream_t st) {
  if (!ne_xi_ok(a.xi, a.ld, a.E, a.A, a.N) || a.ctr == nullptr || a.every < 1 || a.stream < 0 ||
      a.stream >= NZ_STREAMS)
    return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)a.E * xi_off(a.A, a.N).K;
  noisy_env_draw_kernel<<<(unsigned)((n + NE_NT - 1) / NE_NT), NE_NT, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}

APEX_EXPORT int apex_noisy_env_fc(NoisyEnvFc a, hipStream_t st) {
  // (the fc parts of the draw do not depend on the head's shape: A = N = 1 bounds them)
  if (!ne_xi_ok(a.xi, a.ld, a.E, 1, 1)) return (int)hipErrorInvalidValue;
  if (a.X == nullptr || a.W == nullptr || a.S == nullptr || a.bfc == nullptr || a.sbfc == nullptr ||
      a.part == nullptr || a.h == nullptr)
    return (int)hipErrorInvalidValue;
  const bool split = a.X_lo != nullptr;
  if (split != (a.W_lo != nullptr) || split != (a.S_lo != nullptr) || split != (a.h_lo != nullptr))
    return (int)hipErrorInvalidValue;
  if (a.ksplit != noisy_env_ksplit(a.E) || a.n_part < (int64_t)a.ksplit * 2 * a.E * NZ_FC_OUT)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)a.X | (uintptr_t)a.X_lo | (uintptr_t)a.W | (uintptr_t)a.W_lo | (uintptr_t)a.S | (uintptr_t)a.S_lo |
       (uintptr_t)a.bfc | (uintptr_t)a.sbfc | (uintptr_t)a.part | (uintptr_t)a.h | (uintptr_t)a.h_lo) & 15)
    return (int)hipErrorInvalidValue;
  const dim3 grid(NZ_FC_OUT / 64, (unsigned)((a.E + 63) / 64), (unsigned)a.ksplit);
  if (split) noisy_env_fc_kernel<true><<<grid, NE_NT, 0, st>>>(a);
  else noisy_env_fc_kernel<false><<<grid, NE_NT, 0, st>>>(a);
  noisy_env_fc_epilogue_kernel<<<(unsigned)a.E, NE_NT, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}

APEX_EXPORT int apex_noisy_env_logits(NoisyEnvLogits a, hipStream_t st) {
  if (!ne_xi_ok(a.xi, a.ld, a.E, a.A, a.N) || a.H == nullptr || a.L == nullptr) return (int)hipErrorInvalidValue;
  const HeadParams* hp[2] = {&a.mu, &a.sg};
  uintptr_t al = (uintptr_t)a.H | (uintptr_t)a.H_lo | (uintptr_t)a.L;
  for (int i = 0; i < 2; ++i) {
    if (hp[i]->wv == nullptr || hp[i]->bv == nullptr || hp[i]->wa == nullptr || hp[i]->ba == nullptr)
      return (int)hipErrorInvalidValue;
    al |= (uintptr_t)hp[i]->wv | (uintptr_t)hp[i]->wa;
  }
  if (al & 15) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.E + 63) / 64), (unsigned)((a.N + 63) / 64 + (a.A * a.N + 63) / 64));
  if (a.H_lo != nullptr) noisy_env_logits_kernel<true><<<grid, NE_NT, 0, st>>>(a);
  else noisy_env_logits_kernel<false><<<grid, NE_NT, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}

APEX_EXPORT int apex_noisy_env_scalar_finish(ActorIO a, const float* L, hipStream_t st) {
  if (!actor_io_ok(a) || L == nullptr) return (int)hipErrorInvalidValue;
  noisy_env_scalar_finish_kernel<<<(unsigned)((a.E + NE_NT - 1) / NE_NT), NE_NT, 0, st>>>(a, L);
  APEX_CHECK_LAUNCH();
}

// sizeof the three argument blocks (which = 0 / 1 / 2) for the ctypes mirrors
APEX_EXPORT int apex_noisy_env_args_size(int which) {
  return which == 0 ? (int)sizeof(NoisyEnvDraw) : which == 1 ? (int)sizeof(NoisyEnvFc) : (int)sizeof(NoisyEnvLogits);
}
