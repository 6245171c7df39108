// What the wide (65 to 256 atoms / quantiles, MFMA) distributional heads share: csrc/qr_wide_head.hip (quantile)
// and csrc/cat_wide_head.hip (categorical, HL-Gauss).  The head weights are read as csrc/dist_head.h reads them: wv
// [N][512], bv [N], wa [A N][512], ba [A N], fp32.  A wide head is three launches on one stream:
//
//   qr_wide_logits_kernel   L [3B][Jp] = H . W^T without biases, v_mfma_f32_16x16x32_bf16, fp32 accumulation
//                           over K = 512.  A block is a tile of 64 activation rows x 64 logit columns; its four
//                           waves take 16 rows each and share the weight tile.  Row tiles [0, ceil(2B / 64)) read
//                           Hon and the online head, the rest Htg and the target head: a tile never straddles
//                           the 2B boundary, a ragged tile clamps its rows on load and skips them on store.
//                           Column tiles [0, ceil(N / 64)) are value columns (x h[:512]), the rest advantage
//                           columns (x h[512:]); a ragged tile clamps its weight rows and skips the stores.
//                           The fp32 weights are split into bf16 hi + lo on the way into a swizzled LDS tile
//                           (64 rows x 64 k per K slab, 16-byte stores, every element converted once per block);
//                           a wave's activation fragments come straight from the bf16 planes (16-byte loads: each
//                           wave reads only its own rows).  Products: Whi Hhi + Wlo Hhi + Whi Hlo with hi / lo
//                           activation planes, Whi H + Wlo H with one plane.  The next K slab (weights and
//                           activations) is loaded while the current one is multiplied; one barrier per slab.
//                           MFMA operands: A = weights (D row = logit column), B = activations (D column =
//                           activation row), so a lane ends with four consecutive logits of one row: one
//                           16-byte store.  L row = [N padded to 4 | A N padded to 4] = Jp floats.
//   the finish kernel       the head's own: one wave per sample, lane l owns atoms l, l + 64, .. in NQ = ceil(N / 64)
//                           register sets (QWRow / qw_row / qw_theta below are one logits row's dueling terms in
//                           that mapping); it leaves td_abs, loss, q_out and the dhead row [(A + 1) N]
//   qr_wide_dh_kernel       dH [B][1024] = relu'(h) (dhead . W) per stream as an MFMA GEMM: a block is 32 samples
//                           x 64 columns of one stream, K = N (value) or A N (advantage) in slabs of 64 summed in
//                           increasing order inside the block (no split of K, no atomics).  The weight slab
//                           [64 j][64 k] is split to bf16 hi + lo into a K-major LDS image (swz_tr) and read as
//                           transposed fragments (ds_read_b64_tr_b16); dhead is split in registers.  Products
//                           Whi Dhi + Whi Dlo + Wlo Dhi.  A = weights (D row = column k), B = dhead (D column =
//                           sample): a lane ends with four consecutive columns of one sample and stores them as
//                           packed bf16 (or hi / lo planes through split_pk_bf16_h).
//
// Both kernels need only the HeadIO block, N and L.  They are `static`: each of the two translation units carries
// its own copy, compiled with its own flags (ops/build.py SOURCE_FLAGS).  Nothing depends on the order blocks run
// in (no float atomics).
#pragma once
#include "dist_head.h"
#include "mfma_common.h"

#define QW_NT 256       // threads of every kernel here (4 waves)
#define QW_HS 512
#define QW_TILE 8192    // bytes of one 64 x 64 bf16 LDS tile


// What the logits kernel takes: up to two row sets (activation planes, their head, their row count); set 1 follows
// set 0 in L.
struct QWLogits {
  const bf16_t* H0; const bf16_t* H0lo; HeadParams P0; int rows0;
  const bf16_t* H1; const bf16_t* H1lo; HeadParams P1; int rows1;
  int A, N;
  float* L;
};

__host__ __device__ __forceinline__ int qw_nv4(int N) { return (N + 3) & ~3; }
__host__ __device__ __forceinline__ int qr_wide_jp(int A, int N) { return qw_nv4(N) + ((A * N + 3) & ~3); }

__device__ __forceinline__ bf16x8 qw_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

// 8 fp32 -> 8 bf16 hi and 8 bf16 lo
__device__ __forceinline__ void qw_split8(const float4& x, const float4& y, uint4& hi, uint4& lo) {
  split_pk_bf16(x.x, x.y, hi.x, lo.x);
  split_pk_bf16(x.z, x.w, hi.y, lo.y);
  split_pk_bf16(y.x, y.y, hi.z, lo.z);
  split_pk_bf16(y.z, y.w, hi.w, lo.w);
}

// ------------------------------------------------------------------------------------------------ logits
static __global__ void __launch_bounds__(QW_NT) qr_wide_logits_kernel(QWLogits a) {
  __shared__ __attribute__((aligned(16))) uint8_t Ws[2][2][QW_TILE];      // [stage][hi, lo]: 64 weight rows x 64 k
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = a.N, AN = a.A * N, Nv4 = qw_nv4(N), Jp = qr_wide_jp(a.A, N);
  // the row tile: set 0's tiles first
  const int t0 = (a.rows0 + 63) >> 6;
  const bool s1 = (int)blockIdx.x >= t0;
  const bf16_t* __restrict__ H = s1 ? a.H1 : a.H0;
  const bf16_t* __restrict__ Hlo = s1 ? a.H1lo : a.H0lo;
  const int rows = s1 ? a.rows1 : a.rows0;
  const int r_loc = ((int)blockIdx.x - (s1 ? t0 : 0)) * 64 + wv * 16 + (lane & 15);
  const int r_ld = min(r_loc, rows - 1);
  // the column tile: value tiles first
  const int cv = (N + 63) >> 6;
  const bool val = (int)blockIdx.y < cv;
  const int c0 = ((int)blockIdx.y - (val ? 0 : cv)) * 64;
  const int clim = val ? N : AN;
  const float* __restrict__ W = val ? (s1 ? a.P1.wv : a.P0.wv) : (s1 ? a.P1.wa : a.P0.wa);
  const bool split = Hlo != nullptr;

  // staging: thread = weight row tid / 4, 16 consecutive k (two 16-byte chunks of the bf16 row)
  const int wr = tid >> 2, seg = tid & 3;
  const float* __restrict__ wsrc = W + (int64_t)min(c0 + wr, clim - 1) * QW_HS + seg * 16;
  const int64_t hoff = (int64_t)r_ld * (2 * QW_HS) + (val ? 0 : QW_HS) + 8 * (lane >> 4);
  const bf16_t* __restrict__ hsrc = H + hoff;
  const bf16_t* __restrict__ hsrc_lo = split ? Hlo + hoff : nullptr;

  float4 wn[4];
  uint4 hh[2], hl[2], hhn[2], hln[2];
  auto load_slab = [&](int s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) wn[i] = *reinterpret_cast<const float4*>(wsrc + s * 64 + 4 * i);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      hhn[kk] = *reinterpret_cast<const uint4*>(hsrc + s * 64 + 32 * kk);
      hln[kk] = split ? *reinterpret_cast<const uint4*>(hsrc_lo + s * 64 + 32 * kk) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_slab = [&](int stage) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      uint4 hi, lo;
      qw_split8(wn[2 * c], wn[2 * c + 1], hi, lo);
      const int off = swz_row(wr, 2 * seg + c);
      *reinterpret_cast<uint4*>(&Ws[stage][0][off]) = hi;
      *reinterpret_cast<uint4*>(&Ws[stage][1][off]) = lo;
    }
  };

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int NS = QW_HS / 64;
  load_slab(0);
  store_slab(0);
  __syncthreads();
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) { hh[kk] = hhn[kk]; hl[kk] = hln[kk]; }
    if (s + 1 < NS) load_slab(s + 1);
    const int stage = s & 1;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8 xh = qw_frag(hh[kk]), xl = qw_frag(hl[kk]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int off = swz_row(16 * t + (lane & 15), 4 * kk + (lane >> 4));
        const bf16x8 wh = qw_frag(*reinterpret_cast<const uint4*>(&Ws[stage][0][off]));
        const bf16x8 wl = qw_frag(*reinterpret_cast<const uint4*>(&Ws[stage][1][off]));
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, acc[t], 0, 0, 0);
        if (split) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, acc[t], 0, 0, 0);
      }
    }
    // the other stage was last read before the previous barrier
    if (s + 1 < NS) store_slab(stage ^ 1);
    __syncthreads();
  }
  if (r_loc >= rows) return;
  float* __restrict__ Lrow = a.L + (int64_t)((s1 ? a.rows0 : 0) + r_loc) * Jp + (val ? 0 : Nv4);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cb = c0 + 16 * t + 4 * (lane >> 4);
    if (cb + 3 < clim) {
      *reinterpret_cast<float4*>(Lrow + cb) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (cb + i < clim) Lrow[cb + i] = acc[t][i];
    }
  }
}

// ------------------------------------------------------------------------------------------------ rows
// One logits row's dueling terms for this lane's NQ quantiles (i = 64 s + lane; 0 past N): v = value logit +
// bias, mean = the mean over the actions of (advantage + bias), summed in increasing a as dist_row does.
template <int NQ>
struct QWRow {
  const float* L;       // the row (value part at 0, advantage part at Nv4)
  const float* ba;
  float v[NQ], mean[NQ];
};

template <int NQ>
__device__ __forceinline__ QWRow<NQ> qw_row(const float* __restrict__ L, const HeadParams& P, int A, int N, int lane) {
  QWRow<NQ> r;
  r.L = L + qw_nv4(N);
  r.ba = P.ba;
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    const int i = 64 * s + lane;
    const bool ok = i < N;
    r.v[s] = ok ? L[i] + P.bv[i] : 0.f;
    float m = 0.f;
    for (int j = 0; j < A; ++j) m += ok ? r.L[j * N + i] + r.ba[j * N + i] : 0.f;
    r.mean[s] = m / (float)A;
  }
  return r;
}

// quantile 64 s + lane of action j (0 past N)
template <int NQ>
__device__ __forceinline__ float qw_theta(const QWRow<NQ>& r, int j, int s, int N, int lane) {
  const int i = 64 * s + lane;
  return i < N ? r.v[s] + (r.L[j * N + i] + r.ba[j * N + i]) - r.mean[s] : 0.f;
}

// ------------------------------------------------------------------------------------------------ dH
static __global__ void __launch_bounds__(QW_NT) qr_wide_dh_kernel(HeadIO a, int N) {
  __shared__ __attribute__((aligned(16))) uint8_t Wi[2][2][QW_TILE];      // [stage][hi, lo]: K-major 64 j x 64 k
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int B = a.B, AN = a.A * N, J = N + AN;
  const int st = blockIdx.y >> 3, kc0 = (blockIdx.y & 7) * 64;            // stream, first column of the block
  const int K = st ? AN : N;
  const float* __restrict__ W = (st ? a.Pon.wa : a.Pon.wv) + kc0;
  const int mt = wv & 1, ch = wv >> 1;                                    // sample tile, column half of the wave
  const int bs = blockIdx.x * 32 + mt * 16 + (lane & 15);
  const float* __restrict__ drow = a.dhead + (int64_t)min(bs, B - 1) * J + (st ? N : 0);
  const bool split = a.lo.Hon != nullptr;

  float4 wn[2][2];
  float dn[2][8], dc[2][8];
  auto load_slab = [&](int s) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {            // task = (row j of the slab, 16-byte chunk of its 64 columns)
      const int task = tid + QW_NT * u, r = task >> 3, c = task & 7;
      const int j = s * 64 + r;
      const float* p = W + (int64_t)min(j, K - 1) * QW_HS + 8 * c;
      const float4 x = *reinterpret_cast<const float4*>(p), y = *reinterpret_cast<const float4*>(p + 4);
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      wn[u][0] = j < K ? x : z;              // rows past K add zeros
      wn[u][1] = j < K ? y : z;
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int jb = s * 64 + 32 * kk + 8 * (lane >> 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) dn[kk][e] = jb + e < K ? drow[jb + e] : 0.f;
    }
  };
  auto store_slab = [&](int stage) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int task = tid + QW_NT * u, r = task >> 3, c = task & 7;
      uint4 hi, lo;
      qw_split8(wn[u][0], wn[u][1], hi, lo);
      *reinterpret_cast<uint4*>(&Wi[stage][0][swz_tr(r, c)]) = hi;
      *reinterpret_cast<uint4*>(&Wi[stage][1][swz_tr(r, c)]) = lo;
    }
  };

  f32x4 acc[2];
  acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int NS = (K + 63) >> 6;
  load_slab(0);
  store_slab(0);
  __syncthreads();
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int e = 0; e < 8; ++e) dc[kk][e] = dn[kk][e];
    if (s + 1 < NS) load_slab(s + 1);
    const int stage = s & 1;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint4 dhi, dlo;
      qw_split8(make_float4(dc[kk][0], dc[kk][1], dc[kk][2], dc[kk][3]),
                make_float4(dc[kk][4], dc[kk][5], dc[kk][6], dc[kk][7]), dhi, dlo);
      const bf16x8 xh = qw_frag(dhi), xl = qw_frag(dlo);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const bf16x8 wh = tr_frag8(&Wi[stage][0][0], kk, 16 * (2 * ch + n), lane);
        const bf16x8 wl = tr_frag8(&Wi[stage][1][0], kk, 16 * (2 * ch + n), lane);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, acc[n], 0, 0, 0);
      }
    }
    if (s + 1 < NS) store_slab(stage ^ 1);
    __syncthreads();
  }
  if (bs >= B) return;
  // this lane: sample bs, columns kc0 + 16 (2 ch + n) + 4 (lane >> 4) .. + 3 of stream st, masked by the stream ReLU
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int64_t o = (int64_t)bs * (2 * QW_HS) + st * QW_HS + kc0 + 16 * (2 * ch + n) + 4 * (lane >> 4);
    const uint2 hu = *reinterpret_cast<const uint2*>(a.Hon + o);
    float h[4] = {__uint_as_float(hu.x << 16), __uint_as_float(hu.x & 0xffff0000u), __uint_as_float(hu.y << 16),
                  __uint_as_float(hu.y & 0xffff0000u)};
    if (split) {
      const uint2 hv = *reinterpret_cast<const uint2*>(a.lo.Hon + o);
      h[0] += __uint_as_float(hv.x << 16); h[1] += __uint_as_float(hv.x & 0xffff0000u);
      h[2] += __uint_as_float(hv.y << 16); h[3] += __uint_as_float(hv.y & 0xffff0000u);
    }
    float m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = h[i] > 0.f ? acc[n][i] : 0.f;
    if (split) {
      uint32_t h0, l0, h1, l1;
      split_pk_bf16_h(m[0], m[1], h0, l0);
      split_pk_bf16_h(m[2], m[3], h1, l1);
      *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(a.lo.dH + o) = make_uint2(l0, l1);
    } else {
      *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(pack_bf16x2(m[0], m[1]), pack_bf16x2(m[2], m[3]));
    }
  }
}

// ------------------------------------------------------------------------------------------------ launches
static inline dim3 qw_logits_grid(int rows0, int rows1, int A, int N) {
  return dim3((unsigned)((rows0 + 63) / 64 + (rows1 + 63) / 64), (unsigned)((N + 63) / 64 + (A * N + 63) / 64));
}


// The launches both heads issue around their finish kernel.  Learner: rows [0, 2B) are Hon x the online head, rows
// [2B, 3B) Htg x the target head.  Actor: one weight set on the E env rows.
static inline void qw_launch_head_logits(const HeadIO& io, int N, float* L, hipStream_t st) {
  QWLogits g;
  g.H0 = io.Hon; g.H0lo = io.lo.Hon; g.P0 = io.Pon; g.rows0 = 2 * io.B;
  g.H1 = io.Htg; g.H1lo = io.lo.Htg; g.P1 = io.Ptg; g.rows1 = io.B;
  g.A = io.A; g.N = N; g.L = L;
  qr_wide_logits_kernel<<<qw_logits_grid(g.rows0, g.rows1, g.A, g.N), QW_NT, 0, st>>>(g);
}

static inline void qw_launch_actor_logits(const ActorIO& io, int N, float* L, hipStream_t st) {
  QWLogits g;
  g.H0 = io.H; g.H0lo = io.H_lo; g.P0 = io.P; g.rows0 = io.E;
  g.H1 = io.H; g.H1lo = io.H_lo; g.P1 = io.P; g.rows1 = 0;
  g.A = io.A; g.N = N; g.L = L;
  qr_wide_logits_kernel<<<qw_logits_grid(g.rows0, 0, g.A, g.N), QW_NT, 0, st>>>(g);
}

static inline void qw_launch_dh(const HeadIO& io, int N, hipStream_t st) {
  qr_wide_dh_kernel<<<dim3((unsigned)((io.B + 31) / 32), 16), QW_NT, 0, st>>>(io, N);
}

// head_io_ok / actor_io_ok plus what the wide launchers share of their own: the N range, the stream width, the
// workspace, and 16-byte loads of the activation planes and stores of the logits.  Every kernel of a wide head uses
// 32 KiB of static LDS or none, inside the default bound for any admitted shape.
static inline bool qw_head_ok(const HeadIO& a, int N, const float* L) {
  if (!head_io_ok(a) || N < 2 || N > 256 || a.hidden != QW_HS || L == nullptr) return false;
  return (((uintptr_t)a.Hon | (uintptr_t)a.Htg | (uintptr_t)a.lo.Hon | (uintptr_t)a.lo.Htg | (uintptr_t)L) & 15) == 0;
}
static inline bool qw_actor_ok(const ActorIO& a, int N, const float* L) {
  if (!actor_io_ok(a) || N < 2 || N > 256 || a.hidden != QW_HS || L == nullptr) return false;
  return (((uintptr_t)a.H | (uintptr_t)a.H_lo | (uintptr_t)L) & 15) == 0;
}
