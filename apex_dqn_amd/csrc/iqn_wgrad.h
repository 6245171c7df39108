// Weight gradients of the implicit quantile head (csrc/iqn_head.hip) from what iqn_head_kernel leaves, as a block
// body: csrc/sumtree.hip runs it as blocks of iqn_wgrad_prio_kernel, beside the single-block priority write-back
// (where head_wgrad_prio_kernel runs the wide head's weight gradient for the other distributional heads).
//   G[wv] = sum_b xg_b[:HS]      G[wa][a] = sum_b coef_a(b) xg_b[HS:]     G[bv], G[ba] from gsum
//   G[btau] = sum_{b,k} dpre     G[wtau] = sum_{b,k} dpre (x) cos         coef_a(b) = [a = a_b] - 1/A
// Every sum runs in a fixed order (no float atomics): the result does not depend on the order blocks run in.
#pragma once
#include "dist_head.h"

#define IQN_E 64         // cosines
#define IQN_WG_CT 16     // embedding rows (columns c of h) per block
#define IQN_WG_AT 8      // actions per head block
#define IQN_WG_S 8       // blocks that split the B N rows of one embedding tile

struct IqnWgArgs {
  const float* dpre;    // [B][N][2 HS]
  const float* cosT;    // [B][N][64]
  const float* xg;      // [B][2 HS]
  const float* gsum;    // [B]
  const int32_t* act;
  int B, A, N;
  float* gwv;           // [HS]
  float* gbv;           // [1]
  float* gwa;           // [A][HS]
  float* gba;           // [A]
  float* gwtau;         // [2 HS][64]
  float* gbtau;         // [2 HS]
  float* part;          // [IQN_WG_S][2 HS 64 + 2 HS] partials of G[wtau | btau]
};

// One net's cosine embedding and iqn_actor_head_kernel's arguments: here, where apex_abi_struct_sizes sees them
struct IqnEmbed {
  const float* w;       // We [2 HS][64]
  const float* b;       // be [2 HS]
};

struct IqnActorArgs {
  ActorIO io;           // seed / ctr: the epsilon-greedy draw's (actor_head_kernel's words)
  IqnEmbed Em;
  int K, midpoint;      // midpoint 1: tau_k = (2 k + 1) / (2 K), no draw
  uint64_t seed_q;
  const int64_t* tau_ctr;   // t: c = 64 t + stream
  int stream;
  float* tau_out;       // [E][K] or null
};
static_assert(std::is_standard_layout_v<IqnActorArgs> && std::is_trivially_copyable_v<IqnActorArgs>);

static inline int iqn_wgrad_blocks(int A) {
  return IQN_WG_S * (2 * DIST_HS / IQN_WG_CT) + (1 + (A + IQN_WG_AT - 1) / IQN_WG_AT) * (DIST_HS / 64);
}

// block `blk` of iqn_wgrad_blocks(A), 512 threads.
// blocks [0, 8 * 2 HS / 16): (tile, split): a 16 x 64 tile of G[wtau] (+ 16 of G[btau]) over the rows b k = 64 i +
// 8 split + w of wave w; lane (cq, ig) holds columns 4 cq .. + 3 against cosines 4 ig .. + 3; the eight wave
// partials meet in LDS and are added in wave order, the block's sum goes to its split's partial plane, and
// iqn_wgrad_reduce_body (a small second launch) adds the eight planes in split order.  (The tile's last-arriving
// block adding them behind a device-scope fence saved that launch and cost 110 us: docs/PERF_NOTES.md.)
// blocks after: (tile, chunk) of the heads: tile 0 the value row, tile 1 + t actions 8 t .. + 7; chunk = 64
// columns; wave w sums samples w, w + 8, ..
__device__ __forceinline__ void iqn_wgrad_body(const IqnWgArgs& h, int blk) {
  __shared__ __attribute__((aligned(16))) float red[8][IQN_WG_CT * IQN_E + 64];
  constexpr int HS = DIST_HS, ROW = 2 * HS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int B = h.B, A = h.A, N = h.N;
  const int nt = ROW / IQN_WG_CT;
  if (blk < nt * IQN_WG_S) {
    const int tile = blk / IQN_WG_S, c0 = tile * IQN_WG_CT, sp = blk % IQN_WG_S;
    const int cq = lane >> 4, ig = lane & 15;
    float acc[4][4], accb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      accb[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    }
    const int K = B * N;
    const float* __restrict__ dp = h.dpre + c0 + 4 * cq;
    const float* __restrict__ cp = h.cosT + 4 * ig;
#pragma unroll 8
    for (int r = sp * 8 + w; r < K; r += 8 * IQN_WG_S) {
      const float4 d = *reinterpret_cast<const float4*>(dp + (int64_t)r * ROW);
      const float4 c = *reinterpret_cast<const float4*>(cp + (int64_t)r * IQN_E);
      const float dv[4] = {d.x, d.y, d.z, d.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        accb[i] += dv[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(dv[i], cv[j], acc[i][j]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<float4*>(&red[w][(4 * cq + i) * IQN_E + 4 * ig]) =
          make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
      if (ig == 0) red[w][IQN_WG_CT * IQN_E + 4 * cq + i] = accb[i];
    }
    __syncthreads();
    constexpr int64_t plane = (int64_t)ROW * IQN_E + ROW;
    for (int o = tid; o < IQN_WG_CT * IQN_E + IQN_WG_CT; o += 512) {
      float s = red[0][o];
#pragma unroll
      for (int q = 1; q < 8; ++q) s += red[q][o];
      float* part = h.part + (int64_t)sp * plane;
      if (o < IQN_WG_CT * IQN_E) part[(int64_t)c0 * IQN_E + o] = s;
      else part[ROW * IQN_E + c0 + o - IQN_WG_CT * IQN_E] = s;
    }
    return;
  }
  const int hb = blk - nt * IQN_WG_S;
  const int tile = hb >> 3, chunk = hb & 7;
  const int col = chunk * 64 + lane;
  const float invA = 1.0f / (float)A;
  float acc[IQN_WG_AT], accb[IQN_WG_AT];
#pragma unroll
  for (int t = 0; t < IQN_WG_AT; ++t) acc[t] = accb[t] = 0.f;
  const int a0 = (tile - 1) * IQN_WG_AT;
  if (tile == 0) {
#pragma unroll 4
    for (int b = w; b < B; b += 8) {
      acc[0] += h.xg[(int64_t)b * ROW + col];
      accb[0] += h.gsum[b];
    }
  } else {
#pragma unroll 4
    for (int b = w; b < B; b += 8) {
      const float x = h.xg[(int64_t)b * ROW + HS + col];
      const float gs = h.gsum[b];
      const int ab = h.act[b];
#pragma unroll
      for (int t = 0; t < IQN_WG_AT; ++t) {
        const float cf = (ab == a0 + t ? 1.f : 0.f) - invA;
        acc[t] = fmaf(cf, x, acc[t]);
        accb[t] = fmaf(cf, gs, accb[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < IQN_WG_AT; ++t) {
    red[w][t * 65 + lane] = acc[t];
    if (lane == 0) red[w][t * 65 + 64] = accb[t];
  }
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int t = 0; t < IQN_WG_AT; ++t) {
    float s = 0.f, sb = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      s += red[q][t * 65 + lane];
      sb += red[q][t * 65 + 64];
    }
    if (tile == 0) {
      if (t == 0) {
        h.gwv[col] = s;
        if (lane == 0 && chunk == 0) h.gbv[0] = sb;
      }
    } else if (a0 + t < A) {
      h.gwa[(int64_t)(a0 + t) * HS + col] = s;
      if (lane == 0 && chunk == 0) h.gba[a0 + t] = sb;
    }
  }
}

static inline bool iqn_wgrad_args_ok(const IqnWgArgs& h) {
  if (h.A < 1 || h.A > HEAD_MAXA || h.B < 1 || h.N < 2 || h.N > 64) return false;
  if (h.dpre == nullptr || h.cosT == nullptr || h.xg == nullptr || h.gsum == nullptr || h.act == nullptr ||
      h.gwv == nullptr || h.gbv == nullptr || h.gwa == nullptr || h.gba == nullptr || h.gwtau == nullptr ||
      h.gbtau == nullptr || h.part == nullptr)
    return false;
  return ((((uintptr_t)h.dpre | (uintptr_t)h.cosT) & 15) == 0);
}

// G[wtau | btau] = the IQN_WG_S partial planes added in split order; one thread per value
__device__ __forceinline__ void iqn_wgrad_reduce_body(const IqnWgArgs& h, int o) {
  constexpr int n = 2 * DIST_HS * IQN_E + 2 * DIST_HS;
  if (o >= n) return;
  float s = h.part[o];
#pragma unroll
  for (int q = 1; q < IQN_WG_S; ++q) s += h.part[(int64_t)q * n + o];
  if (o < 2 * DIST_HS * IQN_E) h.gwtau[o] = s;
  else h.gbtau[o - 2 * DIST_HS * IQN_E] = s;
}
