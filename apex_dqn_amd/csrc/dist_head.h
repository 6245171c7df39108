// The work the distributional heads share (csrc/c51_head.hip: categorical, csrc/qr_head.hip:
// quantile regression).  Both read the head weights as wv [N][HS], bv [N], wa [A N][HS] (row
// a N + i = action a, atom / quantile i), ba [A N]; HS = 512, N <= 64 (lane = atom), and both
// leave dhead [B][(A + 1) N] and dH.  A head kernel is one block of DIST_NT threads per
// DIST_SPB samples, and its body is dist_head_frame: the LDS carve-up, the phases below with
// their barriers, and between phases 1 and 3 the head's own phase 2, a callable the kernel
// hands in.  A kernel is its shared-memory declaration, that call and its phase 2.
//
//   dist_head_side     zeroes the head-gradient region, leaves the batch-max IS statistic
//   dist_head_stage    phase 0: the 3 DIST_SPB activation rows (online S_t, online S_t+n,
//                      target S_t+n; hi + lo in split mode) -> LDS as fp32
//   dist_head_logits   phase 1: the (A + 1) N logits of every staged row, without biases.
//                      Every wave takes weight rows four at a time: 16 lanes per row, lane l
//                      of them columns 64 c + 4 l .. + 3 (c = 0..7) as eight float4 loads --
//                      each load instruction reads four 256-B runs -- multiplies them with
//                      every staged row of that weight set (ds_read_b128, the four 16-lane
//                      groups read the same addresses) and reduces within its 16 lanes by
//                      four DPP steps.  A block reads both weight sets once for DIST_SPB
//                      samples; the next group's weights are loaded while the current one
//                      is multiplied.
//   phase 2            wave s finishes sample s with lane = atom: the frame reads the sample's
//                      row of the batch (DistSample), calls the head's callable for td_abs,
//                      loss, q_out and this lane's g, and leaves the dhead row in memory and in
//                      LDS over the consumed S_t logits (dist_head_store_dhead)
//   dist_head_dh       phase 3: dH for the block's samples: the threads form four groups of
//                      128, a thread holds four columns, group q adds rows q, q + 4, .. of
//                      dhead . W (float4 weight loads, the coefficients broadcast from LDS);
//                      the groups' partials are added through LDS in a fixed order.
//
// `a` is the kernel's shared argument block (head_common.h HeadIO), N its atom / quantile
// count.  Nothing depends on the order blocks run in (no float atomics).
// dist_actor_logits is phase 1 for the actor heads: one wave per env row, the row in
// registers.
#pragma once
#include "head_common.h"

#define DIST_SPB 2      // samples per block
#define DIST_NT 512     // 8 waves
#define DIST_HS 512

// sum over each 16-lane row (every lane of the row holds it)
__device__ __forceinline__ float row16_sum(float v) {
  APEX_DPP_ADD(v, 0xB1);   // quad_perm(1,0,3,2)
  APEX_DPP_ADD(v, 0x4E);   // quad_perm(2,3,0,1)
  APEX_DPP_ADD(v, 0x124);  // row_ror:4
  APEX_DPP_ADD(v, 0x128);  // row_ror:8
  return v;
}

// the 8 float4 of weight row `wrow` this lane multiplies (columns 64 c + 4 l16 ..)
__device__ __forceinline__ void dist_load_w(const float* __restrict__ wrow, int l16, float4* w) {
#pragma unroll
  for (int c = 0; c < 8; ++c) w[c] = *reinterpret_cast<const float4*>(wrow + c * 64 + l16 * 4);
}

__device__ __forceinline__ float dist_dot(const float4* w, const float4* h) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    acc = fmaf(w[c].x, h[c].x, acc);
    acc = fmaf(w[c].y, h[c].y, acc);
    acc = fmaf(w[c].z, h[c].z, acc);
    acc = fmaf(w[c].w, h[c].w, acc);
  }
  return acc;
}

// Weight-row groups of one weight set: [0, gv) value rows, [gv, gv + ga) advantage rows,
// four rows each (the last group of a stream clamps its row; the store skips it).
struct DistGroup {
  const float* wrow;   // this lane's weight row
  int soff;            // stream offset of the activations (0 value, HS advantage)
  int j;               // logit column (N + a N + i for advantages), or -1: no store
};

__device__ __forceinline__ DistGroup dist_group(const HeadParams& P, int u, int gv, int N, int AN, int lane) {
  DistGroup g;
  const int sub = lane >> 4;
  if (u < gv) {
    const int r = u * 4 + sub;
    g.wrow = P.wv + (int64_t)min(r, N - 1) * DIST_HS;
    g.soff = 0;
    g.j = r < N ? r : -1;
  } else {
    const int r = (u - gv) * 4 + sub;
    g.wrow = P.wa + (int64_t)min(r, AN - 1) * DIST_HS;
    g.soff = DIST_HS;
    g.j = r < AN ? N + r : -1;
  }
  return g;
}

// One activation row's dueling terms, lane = atom (valid = lane < N): L = the row's logits
// without biases ([N] value, then [A][N]).
struct DistRow {
  const float* L;
  const float* bv;
  const float* ba;
  float v;      // value logit + bias of this lane's atom
  float mean;   // mean over the actions of (advantage + bias)
};

__device__ __forceinline__ DistRow dist_row(const float* L, const HeadParams& P, int A, int N, int lane) {
  DistRow r;
  r.L = L;
  r.bv = P.bv;
  r.ba = P.ba;
  const bool valid = lane < N;
  r.v = valid ? L[lane] + P.bv[lane] : 0.f;
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += valid ? L[N + a * N + lane] + P.ba[a * N + lane] : 0.f;
  r.mean = s / (float)A;
  return r;
}

// floats of LDS a head kernel needs: [3 SPB][2 HS] activations + [3 SPB][Jp] logits
static inline size_t dist_head_lds(int A, int N) {
  const int J = (A + 1) * N, Jp = (J + 3) & ~3;
  return (size_t)(3 * DIST_SPB) * (2 * DIST_HS + Jp) * sizeof(float);
}

__device__ __forceinline__ void dist_head_side(const HeadIO& a, int tid, int lane, int wv) {
  // zero the head-gradient region that the head weight gradient accumulates into
  if (a.zero_ptr != nullptr)
    for (int i = blockIdx.x * DIST_NT + tid; i < a.zero_n; i += gridDim.x * DIST_NT) a.zero_ptr[i] = 0.f;
  // batch-max IS statistic (ddqn_head_kernel's): block 0's last wave
  if ((a.isn.out != nullptr || a.isn.valid_count != nullptr) && blockIdx.x == 0 && wv == DIST_NT / 64 - 1)
    head_is_norm(a, lane);
}

// ---- phase 0: the block's activation rows -> LDS (fp32; a sample past the batch reads the last row)
// Hs [3 SPB][ROW]: rows s (S_t), SPB + s (online S_t+n), 2 SPB + s (target)
__device__ __forceinline__ void dist_head_stage(const HeadIO& a, float* Hs, int b0, int tid, bool split) {
  constexpr int HS = DIST_HS, ROW = 2 * HS, SPB = DIST_SPB, NR = 3 * SPB;
  const int B = a.B;
  for (int r = 0; r < NR; ++r) {
    const int s = r % SPB, kind = r / SPB;
    const int b = min(b0 + s, B - 1);
    const int64_t off = (kind == 1 ? (int64_t)(B + b) : (int64_t)b) * ROW;
    const bf16_t* src = (kind == 2 ? a.Htg : a.Hon) + off;
    const uint32_t u = reinterpret_cast<const uint32_t*>(src)[tid];          // columns 2 tid, 2 tid + 1
    float x0 = __uint_as_float(u << 16), x1 = __uint_as_float(u & 0xffff0000u);
    if (split) {
      const bf16_t* sl = (kind == 2 ? a.lo.Htg : a.lo.Hon) + off;
      const uint32_t v = reinterpret_cast<const uint32_t*>(sl)[tid];
      x0 += __uint_as_float(v << 16);
      x1 += __uint_as_float(v & 0xffff0000u);
    }
    *reinterpret_cast<float2*>(Hs + r * ROW + 2 * tid) = make_float2(x0, x1);
  }
}

// ---- phase 1: logits of every staged row -> Ls [3 SPB][Jp] (no biases)
__device__ __forceinline__ void dist_head_logits(const HeadIO& a, int N, const float* Hs, float* Ls, int Jp, int lane,
                                                 int wv) {
  constexpr int HS = DIST_HS, ROW = 2 * HS, SPB = DIST_SPB;
  const int AN = a.A * N;
  const int l16 = lane & 15;
  const int gv = (N + 3) >> 2, ga = (AN + 3) >> 2, G1 = gv + ga;
  constexpr int NW = DIST_NT / 64;
  float4 w[8], wn[8];
  int t = wv;
  DistGroup g{a.Pon.wv, 0, -1};
  if (t < 2 * G1) {       // (a tiny head has fewer tasks than waves)
    g = dist_group(t >= G1 ? a.Ptg : a.Pon, t >= G1 ? t - G1 : t, gv, N, AN, lane);
    dist_load_w(g.wrow, l16, w);
  }
  for (; t < 2 * G1; t += NW) {
    const int tn = t + NW;
    DistGroup gn = g;
    if (tn < 2 * G1) {
      gn = dist_group(tn >= G1 ? a.Ptg : a.Pon, tn >= G1 ? tn - G1 : tn, gv, N, AN, lane);
      dist_load_w(gn.wrow, l16, wn);
    }
    const bool tg = t >= G1;
    const int r0 = tg ? 2 * SPB : 0, nr = tg ? SPB : 2 * SPB;
    for (int rr = 0; rr < nr; ++rr) {
      const float* hrow = Hs + (r0 + rr) * ROW + g.soff + l16 * 4;
      float4 h[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) h[c] = *reinterpret_cast<const float4*>(hrow + c * 64);
      const float acc = row16_sum(dist_dot(w, h));
      if (l16 == 0 && g.j >= 0) Ls[(r0 + rr) * Jp + g.j] = acc;
    }
    g = gn;
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = wn[c];
  }
}

// The dhead row of a sample (lane = atom, g = d loss / d logit of the taken action's atom):
// to memory, and into LDS (D: over the consumed S_t logits) for phase 3.  A dead sample
// (past the batch) stores nothing to memory and zeros to LDS.
__device__ __forceinline__ void dist_head_store_dhead(float g, bool live, bool valid, int a_b, int A, int N, int lane,
                                                      float* D, float* dh) {
  const float invA = 1.0f / (float)A;
  const float gl = live ? g : 0.f;
  if (valid) {
    D[lane] = gl;
    if (live) dh[lane] = g;
    for (int j = 0; j < A; ++j) {
      const float c = (j == a_b ? 1.f : 0.f) - invA;
      D[N + j * N + lane] = gl * c;
      if (live) dh[N + j * N + lane] = g * c;
    }
  }
}

// ---- phase 3: dH[s][k] = relu'(h) sum_j dhead[s][j] W[j][k]  (contains block barriers)
__device__ __forceinline__ void dist_head_dh(const HeadIO& a, int N, float* Hs, const float* Ls, int Jp, int b0, int tid,
                                             bool split) {
  constexpr int HS = DIST_HS, ROW = 2 * HS, SPB = DIST_SPB;
  const int B = a.B, AN = a.A * N;
  const int q = tid >> 7, ct = tid & 127;       // row group, column quad
  float4 av[SPB], aa[SPB];
#pragma unroll
  for (int s = 0; s < SPB; ++s) av[s] = aa[s] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* __restrict__ wvp = a.Pon.wv + ct * 4;
  const float* __restrict__ wap = a.Pon.wa + ct * 4;
#pragma unroll 4
  for (int j = q; j < N; j += 4) {
    const float4 w = *reinterpret_cast<const float4*>(wvp + (int64_t)j * HS);
#pragma unroll
    for (int s = 0; s < SPB; ++s) {
      const float c = Ls[s * Jp + j];
      av[s].x = fmaf(c, w.x, av[s].x); av[s].y = fmaf(c, w.y, av[s].y);
      av[s].z = fmaf(c, w.z, av[s].z); av[s].w = fmaf(c, w.w, av[s].w);
    }
  }
#pragma unroll 4
  for (int j = q; j < AN; j += 4) {
    const float4 w = *reinterpret_cast<const float4*>(wap + (int64_t)j * HS);
#pragma unroll
    for (int s = 0; s < SPB; ++s) {
      const float c = Ls[s * Jp + N + j];
      aa[s].x = fmaf(c, w.x, aa[s].x); aa[s].y = fmaf(c, w.y, aa[s].y);
      aa[s].z = fmaf(c, w.z, aa[s].z); aa[s].w = fmaf(c, w.w, aa[s].w);
    }
  }
  // the four groups' partials, added in a fixed order through the LDS rows of the
  // S_t+n activations (consumed): (0 += 2, 1 += 3), then 0 += 1
  float4* red = reinterpret_cast<float4*>(Hs + SPB * ROW);      // [2][SPB][2][128] float4
  auto slot = [&](int gq, int s, int st) { return red + ((gq * SPB + s) * 2 + st) * 128 + ct; };
  if (q >= 2) {
#pragma unroll
    for (int s = 0; s < SPB; ++s) { *slot(q - 2, s, 0) = av[s]; *slot(q - 2, s, 1) = aa[s]; }
  }
  __syncthreads();
  if (q < 2) {
#pragma unroll
    for (int s = 0; s < SPB; ++s) {
      const float4 x = *slot(q, s, 0), y = *slot(q, s, 1);
      av[s].x += x.x; av[s].y += x.y; av[s].z += x.z; av[s].w += x.w;
      aa[s].x += y.x; aa[s].y += y.y; aa[s].z += y.z; aa[s].w += y.w;
    }
  }
  __syncthreads();
  if (q == 1) {
#pragma unroll
    for (int s = 0; s < SPB; ++s) { *slot(0, s, 0) = av[s]; *slot(0, s, 1) = aa[s]; }
  }
  __syncthreads();
  if (q == 0) {
#pragma unroll
    for (int s = 0; s < SPB; ++s) {
      if (b0 + s >= B) continue;
      const float4 x = *slot(0, s, 0), y = *slot(0, s, 1);
      float d[2][4] = {{av[s].x + x.x, av[s].y + x.y, av[s].z + x.z, av[s].w + x.w},
                       {aa[s].x + y.x, aa[s].y + y.y, aa[s].z + y.z, aa[s].w + y.w}};
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const float4 hx = *reinterpret_cast<const float4*>(Hs + s * ROW + st * HS + ct * 4);
        const float m0 = hx.x > 0.f ? d[st][0] : 0.f, m1 = hx.y > 0.f ? d[st][1] : 0.f;
        const float m2 = hx.z > 0.f ? d[st][2] : 0.f, m3 = hx.w > 0.f ? d[st][3] : 0.f;
        const int64_t o = (int64_t)(b0 + s) * ROW + st * HS + ct * 4;
        if (split) {
          uint32_t h0, l0, h1, l1;
          split_pk_bf16_h(m0, m1, h0, l0);
          split_pk_bf16_h(m2, m3, h1, l1);
          *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(a.lo.dH + o) = make_uint2(l0, l1);
        } else {
          *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(pack_bf16x2(m0, m1), pack_bf16x2(m2, m3));
        }
      }
    }
  }
}

// What phase 2 is handed: wave s finishes sample s = row b of the batch (a sample past the batch repeats the
// last row with live = false and stores nothing); valid = lane < N.
struct DistSample {
  int s, b, a_b;
  bool live, valid;
  float rew, gam, w;    // R, Gamma and the IS weight (1 without one) of row b
};

// A head kernel's body.  `smem`: dist_head_lds floats.  `finish(d, Ls, Jp, lane)` is the head's phase 2 for one
// sample: rows d.s, SPB + d.s and 2 SPB + d.s of Ls [3 SPB][Jp] hold the logits of S_t, online S_t+n and target
// S_t+n; it stores td_abs, loss and q_out of a live sample and returns this lane's g.
template <class Finish>
__device__ __forceinline__ void dist_head_frame(const HeadIO& a, int N, float* smem, Finish finish) {
  constexpr int ROW = 2 * DIST_HS, SPB = DIST_SPB, NR = 3 * SPB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int J = N + a.A * N, Jp = (J + 3) & ~3;
  float* Hs = smem;                      // [NR][ROW]: rows s (S_t), SPB + s (online S_t+n), 2 SPB + s (target)
  float* Ls = smem + NR * ROW;           // [NR][Jp] logits (no biases); rows s later hold the dhead rows
  const int b0 = blockIdx.x * SPB;
  const bool split = a.lo.Hon != nullptr;

  dist_head_side(a, tid, lane, wv);
  dist_head_stage(a, Hs, b0, tid, split);
  __syncthreads();
  dist_head_logits(a, N, Hs, Ls, Jp, lane, wv);
  __syncthreads();

  if (wv < SPB) {
    DistSample d;
    d.s = wv;
    d.live = b0 + d.s < a.B;
    d.b = min(b0 + d.s, a.B - 1);
    d.valid = lane < N;
    d.a_b = a.act[d.b];
    d.rew = a.rew[d.b];
    d.gam = a.gam[d.b];
    d.w = a.isw != nullptr ? a.isw[d.b] : 1.f;
    const float g = finish(d, Ls, Jp, lane);
    dist_head_store_dhead(g, d.live, d.valid, d.a_b, a.A, N, lane, Ls + d.s * Jp, a.dhead + (int64_t)d.b * J);
  }
  __syncthreads();

  dist_head_dh(a, N, Hs, Ls, Jp, b0, tid, split);
}

// head_io_ok plus what the C51 / QR launchers share of their own: the N range, the stream width
// and the LDS bound; the LDS in `lds`.
static inline bool dist_head_args_ok(const HeadIO& a, int N, size_t* lds) {
  if (!head_io_ok(a) || N < 2 || N > 64 || a.hidden != DIST_HS) return false;
  *lds = dist_head_lds(a.A, N);
  return *lds <= 65536;     // (A + 1) N <= 1706 logits per row
}

// How the three launchers close: one block per DIST_SPB samples, the kernel instantiated for value rescaling
// when HeadIO.rescale_eps > 0.
template <class Args>
static inline int dist_head_launch(void (*rescale)(Args), void (*plain)(Args), const Args& a, size_t lds,
                                   hipStream_t st) {
  const int grid = (a.io.B + DIST_SPB - 1) / DIST_SPB;
  (a.io.rescale_eps > 0.f ? rescale : plain)<<<grid, DIST_NT, lds, st>>>(a);
  APEX_CHECK_LAUNCH();
}

// Actor heads: the logits (no biases) of env row `e` -> L [Jp], one wave, the row's
// activations in registers (this lane's columns 64 c + 4 l16 .. + 3 of both streams).
// The caller barriers before it reads L.
__device__ __forceinline__ void dist_actor_logits(const bf16_t* __restrict__ H, const bf16_t* __restrict__ H_lo,
                                                  const HeadParams& P, int e, int A, int N, int lane, float* L) {
  constexpr int HS = DIST_HS, ROW = 2 * HS;
  const int l16 = lane & 15;
  const int AN = A * N;
  float4 hv[8], ha[8];
  {
    const bf16_t* row = H + (int64_t)e * ROW + l16 * 4;
    const bf16_t* row_lo = H_lo != nullptr ? H_lo + (int64_t)e * ROW + l16 * 4 : nullptr;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const uint2 u = *reinterpret_cast<const uint2*>(row + st * HS + c * 64);
        float4 x = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                               __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
        if (row_lo != nullptr) {
          const uint2 v = *reinterpret_cast<const uint2*>(row_lo + st * HS + c * 64);
          x.x += __uint_as_float(v.x << 16); x.y += __uint_as_float(v.x & 0xffff0000u);
          x.z += __uint_as_float(v.y << 16); x.w += __uint_as_float(v.y & 0xffff0000u);
        }
        if (st) ha[c] = x;
        else hv[c] = x;
      }
    }
  }
  const int gv = (N + 3) >> 2, ga = (AN + 3) >> 2;
  for (int u = 0; u < gv; ++u) {
    const DistGroup g = dist_group(P, u, gv, N, AN, lane);
    float4 w[8];
    dist_load_w(g.wrow, l16, w);
    const float acc = row16_sum(dist_dot(w, hv));
    if (l16 == 0 && g.j >= 0) L[g.j] = acc;
  }
  for (int u = gv; u < gv + ga; ++u) {
    const DistGroup g = dist_group(P, u, gv, N, AN, lane);
    float4 w[8];
    dist_load_w(g.wrow, l16, w);
    const float acc = row16_sum(dist_dot(w, ha));
    if (l16 == 0 && g.j >= 0) L[g.j] = acc;
  }
}

// Arguments of the C51 / QR actor heads (csrc/c51_head.hip, csrc/qr_head.hip; ops/_lib.py holds the mirrors)
struct C51ActorArgs {
  ActorIO io;
  int N;
  float vmin, vmax;
};
struct QRActorArgs {
  ActorIO io;
  int N;
};
static_assert(std::is_trivially_copyable_v<C51ActorArgs> && std::is_trivially_copyable_v<QRActorArgs> &&
              std::is_standard_layout_v<C51ActorArgs> && std::is_standard_layout_v<QRActorArgs>);

// actor_io_ok plus what the C51 / QR actor launchers share of their own; the LDS of a block in `lds`
static inline bool dist_actor_args_ok(const ActorIO& a, int N, size_t* lds) {
  *lds = (size_t)4 * (((a.A + 1) * N + 3) & ~3) * sizeof(float);
  return actor_io_ok(a) && N >= 2 && N <= 64 && a.hidden == DIST_HS;
}

// How the C51 / QR actor kernels open: wave wv takes env row e = 4 blockIdx.x + wv (past E: the last row again,
// live = false) and leaves its logits in its slice of `smem`, returned, behind a block barrier.
__device__ __forceinline__ float* dist_actor_open(const ActorIO& a, int N, float* smem, int lane, int wv, int& e,
                                                  bool& live) {
  const int AN = a.A * N, J = N + AN, Jp = (J + 3) & ~3;
  const int e_raw = blockIdx.x * 4 + wv;
  live = e_raw < a.E;
  e = min(e_raw, a.E - 1);
  float* L = smem + wv * Jp;
  dist_actor_logits(a.H, a.H_lo, a.P, e, a.A, N, lane, L);
  __syncthreads();
  return L;
}
