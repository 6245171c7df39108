// Wide implicit quantile (IQN) head: Runtime.iqn_wide with dist_head = "implicit", 2 <= N <= 256 samples per state.
// The definitions are csrc/iqn_head.hip's (c(tau), pre, phi, x, theta, a*, T_j, the quantile Huber loss with its
// j-sums in increasing j, dhead, td_abs, dH, and what iqn_wgrad_prio_kernel consumes); the draws are its draws with
// the row stride 64 for N <= 64 (the same fractions, bit for bit) and 256 above (learner/iqn.py learner_taus).
//
// iqn_head_kernel forms pre = We c + be as 64 dependent fp32 fma per (column, sample) and maps one lane to one
// sample.  Here both products are split-bf16 v_mfma_f32_16x16x32_bf16 GEMMs (operands hi + lo, products hi hi +
// lo hi + hi lo, fp32 accumulation) and a lane owns up to four samples.  Three launches on one stream:
//
//   iqn_wide_logits_kernel   L [3B][Jp] (csrc/wide_head.h's row: [N pad 4 | A N pad 4], column a' N + k), the logits
//                            without biases of the rows online S_t, online S_t+n, target S_t+n.  A block of eight
//                            waves takes one (row, stream) at a time and walks rows blockIdx.x, + gridDim.x, ..; wave
//                            w owns the stream's columns 64 w .. + 63 and keeps their We rows as bf16 hi + lo
//                            A-fragments (64 VGPRs) and its slice of the head weights (32) for the whole walk: they
//                            are loaded again only where the walk passes from the online to the target net.  Per
//                            row the N fractions are drawn, their cosines formed once per block (iqn_cos), split and
//                            staged in LDS as B operands (128-byte rows, swz_row); per tile of 16 samples (the tail
//                            tile clamps its sample on load and skips it on store) a wave runs
//                              pre  [64 c][16 k]  = We c(tau_k)                K = 64: 24 MFMAs
//                              x                  = h relu(pre + be)           in the accumulator registers
//                              part [a'][16 k]    = sum_c W[a', c] x[k, c]     K = 64: 10 MFMAs per 16 rows a'
//                            (W in three bf16 terms, exact: hi hi + mid hi + hi lo + lo hi + mid lo)
//                            The second product takes the first one's D layout (four consecutive columns of one
//                            sample per lane) straight back as a B operand: two column tiles make one K = 32
//                            fragment, and the head-weight A-fragment is loaded under the same column permutation
//                            (a sum over c does not care about its order): no LDS transpose.  The eight waves'
//                            partials meet in LDS and are added in wave order.
//   iqn_wide_finish_kernel   <RESCALE, NQ> one wave per sample, four per block; lane l owns samples l, l + 64, .. in
//                            NQ = ceil(N / 64) register sets: qr_wide_finish_kernel with the drawn tau_i of set 0 in
//                            the place of the midpoints and the head's scalar-shaped biases (bv [1], ba [A]).  Writes
//                            td_abs, loss, q_out, dhead [B][(A + 1) N], gsum, and carries dist_head_side's duties.
//   iqn_wide_bwd_kernel      the B training rows, the logits kernel's walk and first product again (set 0).  The
//                            gradient is rank-1 per sample, dx_k[c] = g_k u[c] with u = wv (value) or sum_a coef_a
//                            wa[a] (advantage), so no second GEMM: with S[c] = sum_k g_k phi_k[c]
//                              dpre [B][N][1024] = [pre_k > 0] g_k u h       cosT [B][N][64]
//                              dH = [h > 0] u S                               xg = h S
//                            S: a lane adds its samples in increasing k, then the 16 lanes of a DPP row are added in
//                            a fixed order.
//
// Munchausen-IQN (dist_head = "implicit_munchausen", apex_miqn_wide_head): the logits kernel's MPLAN instantiation
// (online S_t, target S_t+n, target S_t; the net switch at row B), miqn_wide_finish_kernel in the finish kernel's
// place, the same backward.
//
// Nothing depends on the order blocks run in (no float atomics).
#include "iqn_wgrad.h"
#include "wide_head.h"

#define IQW_NT 512      // eight waves: 64 columns of one stream each
#define IQW_NW 8
#define IQW_MR 32       // rows a' of the head product, padded (two tiles of 16: A <= 32)

struct IqnWideArgs {
  IqnArgs h;            // as iqn_head_kernel's (max_blocks caps the walking grids per stream)
  float* L;             // [3B][Jp] fp32 logits workspace (qr_wide_jp)
};
static_assert(std::is_standard_layout_v<IqnWideArgs> && std::is_trivially_copyable_v<IqnWideArgs>);

__host__ __device__ __forceinline__ int iqw_stride(int N) { return N <= 64 ? 64 : 256; }

// dynamic LDS: the cosine planes [hi, lo][N][128 B], the fractions [256], the wave partials [2][8][32 x 16]
static inline size_t iqw_lds(int N) {
  return (size_t)2 * N * 128 + 256 * sizeof(float) + (size_t)2 * IQW_NW * IQW_MR * 16 * sizeof(float);
}

// This wave's We rows (columns 64 w .. + 63 of stream st) as A-fragments, and be in the D layout
struct IqwEmbed {
  uint4 hi[4][2], lo[4][2];   // [column tile][K half]
  float be[4][4];             // column 16 m + 4 g + i
};

__device__ __forceinline__ void iqw_load_embed(const IqnEmbed& E, int c0, int lane, IqwEmbed& f) {
  const int row = lane & 15, g = lane >> 4;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const float* __restrict__ p = E.w + (int64_t)(c0 + 16 * m + row) * IQN_E + 8 * g;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      qw_split8(*reinterpret_cast<const float4*>(p + 32 * kk), *reinterpret_cast<const float4*>(p + 32 * kk + 4),
                f.hi[m][kk], f.lo[m][kk]);
#pragma unroll
    for (int i = 0; i < 4; ++i) f.be[m][i] = E.b[c0 + 16 * m + 4 * g + i];
  }
}

// this lane's 16 stream activations in the D layout: column c0 + 16 m + 4 g + i of row `row` (hi + lo planes)
__device__ __forceinline__ void iqw_load_h(const bf16_t* __restrict__ H, const bf16_t* __restrict__ Hlo, int64_t row,
                                           int c0, int lane, float (&h)[4][4]) {
  const int64_t o = row * (2 * QW_HS) + c0 + 4 * (lane >> 4);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const uint2 u = *reinterpret_cast<const uint2*>(H + o + 16 * m);
    h[m][0] = __uint_as_float(u.x << 16); h[m][1] = __uint_as_float(u.x & 0xffff0000u);
    h[m][2] = __uint_as_float(u.y << 16); h[m][3] = __uint_as_float(u.y & 0xffff0000u);
    if (Hlo != nullptr) {
      const uint2 v = *reinterpret_cast<const uint2*>(Hlo + o + 16 * m);
      h[m][0] += __uint_as_float(v.x << 16); h[m][1] += __uint_as_float(v.x & 0xffff0000u);
      h[m][2] += __uint_as_float(v.y << 16); h[m][3] += __uint_as_float(v.y & 0xffff0000u);
    }
  }
}

// The N fractions of set `set` of batch row b -> Ts, their cosines as bf16 hi / lo B operands -> Chi / Clo (row k
// = sample k, 16-byte chunk c = cosines 8 c .. + 7, swz_row), and in fp32 to cos_out [N][64] (or null).
// Contains two block barriers; the caller's last barrier stands between the previous row's reads and these writes.
__device__ __forceinline__ void iqw_stage_cos(const IqnArgs& ka, uint64_t cword, int b, int set, int N, float* Ts,
                                              uint8_t* Chi, uint8_t* Clo, float* tau_out, float* cos_out, int tid) {
  if (tid < N) {
    const float tau = apex_uniform(ka.seed_q, cword, (uint64_t)(3 * b + set) * (uint64_t)iqw_stride(N) + (uint64_t)tid);
    Ts[tid] = tau;
    if (tau_out != nullptr) tau_out[((int64_t)b * 3 + set) * N + tid] = tau;
  }
  __syncthreads();
  for (int task = tid; task < N * 8; task += IQW_NT) {
    const int k = task >> 3, c = task & 7;
    const float tau = Ts[k];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = iqn_cos(8 * c + e, tau);
    const float4 x = make_float4(v[0], v[1], v[2], v[3]), y = make_float4(v[4], v[5], v[6], v[7]);
    uint4 hi, lo;
    qw_split8(x, y, hi, lo);
    const int off = swz_row(k, c);
    *reinterpret_cast<uint4*>(Chi + off) = hi;
    *reinterpret_cast<uint4*>(Clo + off) = lo;
    if (cos_out != nullptr) {
      *reinterpret_cast<float4*>(cos_out + (int64_t)k * IQN_E + 8 * c) = x;
      *reinterpret_cast<float4*>(cos_out + (int64_t)k * IQN_E + 8 * c + 4) = y;
    }
  }
  __syncthreads();
}

// pre (without be) of this wave's 64 columns at the 16 samples of tile t: acc[m][i] = column 16 m + 4 g + i of
// sample 16 t + (lane & 15); a sample past N reads the last one
__device__ __forceinline__ void iqw_pre_tile(const IqwEmbed& f, const uint8_t* Chi, const uint8_t* Clo, int t, int N,
                                             int lane, f32x4 (&acc)[4]) {
  const int ks = min(16 * t + (lane & 15), N - 1);
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int off = swz_row(ks, 4 * kk + (lane >> 4));
    const bf16x8 ch = qw_frag(*reinterpret_cast<const uint4*>(Chi + off));
    const bf16x8 cl = qw_frag(*reinterpret_cast<const uint4*>(Clo + off));
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(f.hi[m][kk]), ch, acc[m], 0, 0, 0);
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(f.lo[m][kk]), ch, acc[m], 0, 0, 0);
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(f.hi[m][kk]), cl, acc[m], 0, 0, 0);
    }
  }
}

// Two fp32 -> three packed bf16 terms, v = hi + mid + lo exactly (24 bits).  The head weights take all three: their
// rounding is the same for every sample of every row, so at hi + lo (2^-18) it does not average out of G[wv] / G[wa]
// (tests/test_iqn_wide_cpu.py: 1.6 x the bound on the CPU emulation); the per-sample operands keep two terms.
__device__ __forceinline__ void iqw_split3_pk(float a, float b, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
  hi = cvt_pk_bf16(a, b);
  const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
  mid = cvt_pk_bf16(ra, rb);
  lo = cvt_pk_bf16(ra - __uint_as_float(mid << 16), rb - __uint_as_float(mid & 0xffff0000u));
}

__device__ __forceinline__ uint64_t iqw_cword(const IqnArgs& ka) {
  int64_t u = ka.ctr[0] - (ka.base != nullptr ? ka.base[0] : 0);
  u = u < 0 ? 0 : u;
  return 64ull * (uint64_t)u;
}

// ------------------------------------------------------------------------------------------------ logits
// MPLAN (the Munchausen target, miqn_wide_finish_kernel): rows [0, B) the online net at S_t (set 0), [B, 2B) the
// target net at S_t+n (set 2, the plain plan's draws), [2B, 3B) the target net at S_t (set 1); Hon [B], Htg [2B] read
// at r - B; the one net switch of a walk is at row B.  Every difference is an `if constexpr`.
template <bool MPLAN>
__global__ void __launch_bounds__(IQW_NT) iqn_wide_logits_kernel(IqnWideArgs wa) {
  const IqnArgs& ka = wa.h;
  const HeadIO& a = ka.io;
  extern __shared__ __attribute__((aligned(16))) uint8_t iqw_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4;
  const int B = a.B, A = a.A, N = ka.N, Nv4 = qw_nv4(N), Jp = qr_wide_jp(A, N);
  const int st = blockIdx.y, c0 = st * QW_HS + 64 * wv;       // stream; this wave's first column of h
  const int M = st ? A : 1, MT = (M + 15) >> 4;                // rows a' of the head product, tiles of 16
  uint8_t* Chi = iqw_smem;
  uint8_t* Clo = Chi + N * 128;
  float* Ts = reinterpret_cast<float*>(Clo + N * 128);
  float* Pw = Ts + 256;                                        // [2][NW][MR * 16]
  const uint64_t cword = iqw_cword(ka);
  const int NT = (N + 15) >> 4;

  IqwEmbed f;
  uint4 whi[2][2], wmi[2][2], wlo[2][2];                       // head weights [column-tile pair][row tile], three terms
  int cur = -1, buf = 0;
  for (int r = blockIdx.x; r < 3 * B; r += gridDim.x) {
    const int blk = r < B ? 0 : (r < 2 * B ? 1 : 2), b = r - blk * B;
    const int set = MPLAN ? (3 - blk) % 3 : blk, tg = MPLAN ? blk != 0 : blk == 2;
    if (tg != cur) {
      cur = tg;
      iqw_load_embed(tg ? ka.Etg : ka.Eon, c0, lane, f);
      const HeadParams& P = tg ? a.Ptg : a.Pon;
      // A-fragment of pair p: K slots 0..3 = columns 32 p + 4 g .., slots 4..7 = columns 32 p + 16 + 4 g ..: the
      // order in which two D tiles of the first product make one B fragment
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const int row = 16 * mt + (lane & 15);
          float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
          if (row < M) {
            const float* __restrict__ w = (st ? P.wa + (int64_t)row * QW_HS : P.wv) + 64 * wv + 32 * p + 4 * g;
            x = *reinterpret_cast<const float4*>(w);
            y = *reinterpret_cast<const float4*>(w + 16);
          }
          uint4 &hi = whi[p][mt], &mi = wmi[p][mt], &lo = wlo[p][mt];
          iqw_split3_pk(x.x, x.y, hi.x, mi.x, lo.x);
          iqw_split3_pk(x.z, x.w, hi.y, mi.y, lo.y);
          iqw_split3_pk(y.x, y.y, hi.z, mi.z, lo.z);
          iqw_split3_pk(y.z, y.w, hi.w, mi.w, lo.w);
        }
    }
    float h[4][4];
    iqw_load_h(tg ? a.Htg : a.Hon, tg ? a.lo.Htg : a.lo.Hon, tg ? (MPLAN ? r - B : b) : r, c0, lane, h);
    iqw_stage_cos(ka, cword, b, set, N, Ts, Chi, Clo, st == 0 ? ka.tau_out : nullptr, nullptr, tid);
    float* __restrict__ Lrow = wa.L + (int64_t)r * Jp + (st ? Nv4 : 0);
    for (int t = 0; t < NT; ++t) {
      f32x4 acc[4];
      iqw_pre_tile(f, Chi, Clo, t, N, lane, acc);
      float4 x[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        x[m] = make_float4(h[m][0] * fmaxf(acc[m][0] + f.be[m][0], 0.f), h[m][1] * fmaxf(acc[m][1] + f.be[m][1], 0.f),
                           h[m][2] * fmaxf(acc[m][2] + f.be[m][2], 0.f), h[m][3] * fmaxf(acc[m][3] + f.be[m][3], 0.f));
      f32x4 out[2];
      out[0] = out[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        uint4 xh, xl;
        qw_split8(x[2 * p], x[2 * p + 1], xh, xl);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          if (mt < MT) {
            out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(whi[p][mt]), qw_frag(xh), out[mt], 0, 0, 0);
            out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(wmi[p][mt]), qw_frag(xh), out[mt], 0, 0, 0);
            out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(whi[p][mt]), qw_frag(xl), out[mt], 0, 0, 0);
            out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(wlo[p][mt]), qw_frag(xh), out[mt], 0, 0, 0);
            out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qw_frag(wmi[p][mt]), qw_frag(xl), out[mt], 0, 0, 0);
          }
        }
      }
      // this wave's partial [a'][sample]: lane = sample (lane & 15), rows 16 mt + 4 g + i
      float* pw = Pw + (buf * IQW_NW + wv) * (IQW_MR * 16);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        if (mt < MT) {
#pragma unroll
          for (int i = 0; i < 4; ++i) pw[(16 * mt + 4 * g + i) * 16 + (lane & 15)] = out[mt][i];
        }
      __syncthreads();
      // (the next tile writes the other buffer; the one after it writes this one behind the next barrier)
      {
        const int ap = tid >> 4, k = 16 * t + (tid & 15);
        if (ap < M && k < N) {
          const float* q = Pw + buf * IQW_NW * (IQW_MR * 16) + tid;
          float s = q[0];
#pragma unroll
          for (int w = 1; w < IQW_NW; ++w) s += q[w * (IQW_MR * 16)];
          Lrow[ap * N + k] = s;
        }
      }
      buf ^= 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------ finish
// One logits row's dueling terms for this lane's NQ samples (QWRow's mapping, the scalar head's biases)
template <int NQ>
__device__ __forceinline__ QWRow<NQ> iqw_row(const float* __restrict__ L, const HeadParams& P, int A, int N, int lane) {
  QWRow<NQ> r;
  r.L = L + qw_nv4(N);
  r.ba = P.ba;
  const float bv = P.bv[0];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    const int i = 64 * s + lane;
    const bool ok = i < N;
    r.v[s] = ok ? L[i] + bv : 0.f;
    float m = 0.f;
    for (int j = 0; j < A; ++j) m += ok ? r.L[j * N + i] + r.ba[j] : 0.f;
    r.mean[s] = m / (float)A;
  }
  return r;
}

// theta of action j at this lane's samples -> th; q = their mean over the wave
template <int NQ>
__device__ __forceinline__ float iqw_q(const QWRow<NQ>& r, int j, int N, int lane, float invN, float* th) {
  float p = 0.f;
  const float bj = r.ba[j];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    const int i = 64 * s + lane;
    th[s] = i < N ? r.v[s] + (r.L[j * N + i] + bj) - r.mean[s] : 0.f;
    p += th[s];
  }
  return wave_sum_dpp(p) * invN;
}

// What the finish kernels share once this lane's target samples T (0 past N) stand: the online row b of L (q_out, theta
// of a_b), the pairwise quantile Huber loop against the drawn tau of set 0, td_abs, loss, gsum, dhead, the IS statistic
template <bool RESCALE, int NQ>
__device__ __forceinline__ void iqw_finish_tail(const IqnWideArgs& wa, const float (&T)[NQ], int b, bool live, int lane,
                                                int wv);

template <bool RESCALE, int NQ>
__global__ void __launch_bounds__(QW_NT) iqn_wide_finish_kernel(IqnWideArgs wa) {
  const IqnArgs& ka = wa.h;
  const HeadIO& a = ka.io;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int B = a.B, A = a.A, N = ka.N, Jp = qr_wide_jp(A, N);
  if (a.zero_ptr != nullptr)
    for (int i = blockIdx.x * QW_NT + tid; i < a.zero_n; i += gridDim.x * QW_NT) a.zero_ptr[i] = 0.f;
  const int b_raw = blockIdx.x * 4 + wv;
  const bool live = b_raw < B;
  const int b = min(b_raw, B - 1);
  const float rew = a.rew[b], gam = a.gam[b];
  const float invN = 1.0f / (float)N;
  float th[NQ];
  int astar = 0;
  {
    const QWRow<NQ> rn = iqw_row<NQ>(wa.L + (int64_t)(B + b) * Jp, a.Pon, A, N, lane);
    float best = -3.4e38f;
    for (int j = 0; j < A; ++j) {
      const float q = iqw_q(rn, j, N, lane, invN, th);
      if (q > best) { best = q; astar = j; }
    }
    astar = __builtin_amdgcn_readfirstlane(astar);
  }
  float T[NQ];
  {
    const QWRow<NQ> rg = iqw_row<NQ>(wa.L + (int64_t)(2 * B + b) * Jp, a.Ptg, A, N, lane);
    iqw_q(rg, astar, N, lane, invN, th);
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const bool ok = 64 * s + lane < N;
      if constexpr (RESCALE) T[s] = ok ? value_rescale_target(rew, gam, th[s], a.rescale_eps) : 0.f;
      else T[s] = ok ? rew + gam * th[s] : 0.f;
    }
  }
  iqw_finish_tail<RESCALE, NQ>(wa, T, b, live, lane, wv);
}

template <bool RESCALE, int NQ>
__device__ __forceinline__ void iqw_finish_tail(const IqnWideArgs& wa, const float (&T)[NQ], int b, bool live, int lane,
                                                int wv) {
  const IqnArgs& ka = wa.h;
  const HeadIO& a = ka.io;
  const int A = a.A, N = ka.N, J = (A + 1) * N, Jp = qr_wide_jp(A, N);
  const int a_b = a.act[b];
  const float w = a.isw != nullptr ? a.isw[b] : 1.f;
  const float invN = 1.0f / (float)N, kappa = ka.kappa;
  float th[NQ];
  float th_sa[NQ], q_sa = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) th_sa[s] = 0.f;
  {
    const QWRow<NQ> rt = iqw_row<NQ>(wa.L + (int64_t)b * Jp, a.Pon, A, N, lane);
    for (int j = 0; j < A; ++j) {
      const float q = iqw_q(rt, j, N, lane, invN, th);
      if (a.q_out != nullptr && live && lane == 0) a.q_out[(int64_t)b * A + j] = q;
      if (j == a_b) {
        q_sa = q;
#pragma unroll
        for (int s = 0; s < NQ; ++s) th_sa[s] = th[s];
      }
    }
  }
  // the drawn fractions of set 0 (the logits kernel's words), then this lane's samples against every target
  // sample in increasing j
  const uint64_t cword = iqw_cword(ka);
  float tau[NQ], rho[NQ], c[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    const int i = min(64 * s + lane, N - 1);
    tau[s] = apex_uniform(ka.seed_q, cword, (uint64_t)(3 * b) * (uint64_t)iqw_stride(N) + (uint64_t)i);
    rho[s] = c[s] = 0.f;
  }
  float tsum = 0.f;
#pragma unroll
  for (int sj = 0; sj < NQ; ++sj) {
    const int nj = min(64, N - 64 * sj);
    for (int jj = 0; jj < nj; ++jj) {
      const float Tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T[sj]), jj));
      if constexpr (RESCALE) tsum += Tj;
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        const float u = Tj - th_sa[s];
        const float au = fabsf(u);
        const float wgt = fabsf(tau[s] - (u < 0.f ? 1.f : 0.f));
        rho[s] += wgt * (au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa));
        c[s] += wgt * fminf(fmaxf(u, -kappa), kappa);
      }
    }
  }
  const float sc = invN / kappa;
  float rs = 0.f, ts = 0.f, gp = 0.f, gl[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    const bool ok = 64 * s + lane < N;
    rs += ok ? rho[s] * sc : 0.f;
    ts += T[s];
    gl[s] = ok ? -w * a.grad_scale * (c[s] * sc) : 0.f;
    gp += gl[s];
  }
  const float ls = wave_sum_dpp(rs);
  float et;
  if constexpr (RESCALE) et = tsum * invN;
  else et = wave_sum_dpp(ts) * invN;
  const float gs = wave_sum_dpp(gp);
  if (live && lane == 0) {
    a.td_abs[b] = fabsf(et - q_sa);
    a.loss[b] = w * ls;
    if (ka.gsum != nullptr) ka.gsum[b] = gs;
  }
  if (live) {
    float* __restrict__ dh = a.dhead + (int64_t)b * J;
    const float invA = 1.0f / (float)A;
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const int i = 64 * s + lane;
      if (i >= N) continue;
      dh[i] = gl[s];
      for (int j = 0; j < A; ++j) dh[N + j * N + i] = gl[s] * ((j == a_b ? 1.f : 0.f) - invA);
    }
  }
  if ((a.isn.out != nullptr || a.isn.valid_count != nullptr) && blockIdx.x == 0 && wv == QW_NT / 64 - 1)
    head_is_norm(a, lane);
}

// ------------------------------------------------------------------------------------------------ M-IQN finish
// Munchausen-IQN (Runtime.dist_head = "implicit_munchausen"; learner/losses.py miqn_targets is the definition): the
// logits kernel's M plan left rows b (online S_t), B + b (target S_t+n), 2B + b (target S_t) of L.
struct MiqnWideArgs {
  IqnWideArgs w;
  float alpha, tau, clip;   // bonus scale, softmax temperature, lower clip of tau ln pi
  float* aux;               // [B][2] (bonus, vsoft)
};
static_assert(std::is_standard_layout_v<MiqnWideArgs> && std::is_trivially_copyable_v<MiqnWideArgs>);

// tau ln softmax(g / tau) of the A values g held one per lane (lane j = action j; lanes past A pass anything):
// (g - max g) - tau ln sum_a exp((g - max g) / tau), max-subtracted as csrc/head_common.h's MDQN body, accurate expf /
// logf.  Lanes past A return 0.
__device__ __forceinline__ float miqn_tlp(float g, int A, int lane, float tau) {
  const bool on = lane < A;
  const float m = wave_max(on ? g : -3.4e38f);
  const float c = on ? g - m : 0.f;
  const float s = wave_sum_dpp(on ? expf(c / tau) : 0.f);
  return on ? c - tau * logf(s) : 0.f;
}

// One wave per sample as iqn_wide_finish_kernel.  The two target rows' expectations g1[a] / g0[a] are wave sums over
// each action's theta, kept one action per lane (A <= 32); the softmax terms are wave reductions over those lanes and
// reach the second walk over the S_t+n row as v_readlane broadcasts.  That walk re-reads the A logit rows (the L2
// holds them) instead of keeping A x NQ thetas in registers.
template <int NQ>
__global__ void __launch_bounds__(QW_NT) miqn_wide_finish_kernel(MiqnWideArgs ma) {
  const IqnWideArgs& wa = ma.w;
  const IqnArgs& ka = wa.h;
  const HeadIO& a = ka.io;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int B = a.B, A = a.A, N = ka.N, Jp = qr_wide_jp(A, N);
  if (a.zero_ptr != nullptr)
    for (int i = blockIdx.x * QW_NT + tid; i < a.zero_n; i += gridDim.x * QW_NT) a.zero_ptr[i] = 0.f;
  const int b_raw = blockIdx.x * 4 + wv;
  const bool live = b_raw < B;
  const int b = min(b_raw, B - 1);
  const int a_b = __builtin_amdgcn_readfirstlane(a.act[b]);
  const float rew = a.rew[b], gam = a.gam[b];
  const float invN = 1.0f / (float)N, tau_m = ma.tau;
  float th[NQ];
  // target net at S_t+n: g1, tau ln pi1 and pi1 per lane, then the mixture sum_a pi1[a] (theta[a] - tlp1[a]) per owned
  // sample in increasing a
  float mix[NQ], vsoft;
  {
    const QWRow<NQ> r1 = iqw_row<NQ>(wa.L + (int64_t)(B + b) * Jp, a.Ptg, A, N, lane);
    float g1 = 0.f;
    for (int j = 0; j < A; ++j) {
      const float q = iqw_q(r1, j, N, lane, invN, th);
      if (lane == j) g1 = q;
    }
    const float tl1 = miqn_tlp(g1, A, lane, tau_m);
    const float pi1 = lane < A ? expf(tl1 / tau_m) : 0.f;
    vsoft = wave_sum_dpp(pi1 * (g1 - tl1));
#pragma unroll
    for (int s = 0; s < NQ; ++s) mix[s] = 0.f;
    for (int j = 0; j < A; ++j) {
      const float pj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pi1), j));
      const float tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tl1), j));
      const float bj = r1.ba[j];
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        const int i = 64 * s + lane;
        const float t = i < N ? r1.v[s] + (r1.L[j * N + i] + bj) - r1.mean[s] : 0.f;
        mix[s] += pj * (t - tj);
      }
    }
  }
  // target net at S_t: g0 and the bonus alpha clamp(tau ln pi0[a_b], clip, 0)
  float bonus;
  {
    const QWRow<NQ> r0 = iqw_row<NQ>(wa.L + (int64_t)(2 * B + b) * Jp, a.Ptg, A, N, lane);
    float g0 = 0.f;
    for (int j = 0; j < A; ++j) {
      const float q = iqw_q(r0, j, N, lane, invN, th);
      if (lane == j) g0 = q;
    }
    const float tl0 = miqn_tlp(g0, A, lane, tau_m);
    const float t0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tl0), a_b));
    bonus = ma.alpha * fminf(fmaxf(t0, ma.clip), 0.f);
  }
  float T[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) T[s] = 64 * s + lane < N ? rew + bonus + gam * mix[s] : 0.f;
  if (live && lane == 0) {
    ma.aux[2 * (int64_t)b] = bonus;
    ma.aux[2 * (int64_t)b + 1] = vsoft;
  }
  iqw_finish_tail<false, NQ>(wa, T, b, live, lane, wv);
}

// ------------------------------------------------------------------------------------------------ backward
__global__ void __launch_bounds__(IQW_NT) iqn_wide_bwd_kernel(IqnWideArgs wa) {
  const IqnArgs& ka = wa.h;
  const HeadIO& a = ka.io;
  extern __shared__ __attribute__((aligned(16))) uint8_t iqw_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4;
  const int B = a.B, A = a.A, N = ka.N, J = (A + 1) * N;
  const int st = blockIdx.y, c0 = st * QW_HS + 64 * wv;
  uint8_t* Chi = iqw_smem;
  uint8_t* Clo = Chi + N * 128;
  float* Ts = reinterpret_cast<float*>(Clo + N * 128);
  const uint64_t cword = iqw_cword(ka);
  const int NT = (N + 15) >> 4;
  const bool split = a.lo.Hon != nullptr;
  const float invA = 1.0f / (float)A;

  IqwEmbed f;
  iqw_load_embed(ka.Eon, c0, lane, f);
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    float h[4][4], u[4][4], S[4][4];
    iqw_load_h(a.Hon, a.lo.Hon, b, c0, lane, h);
    // u: wv, or sum_a coef_a wa[a] in increasing a (coef_a = [a = a_b] - 1 / A)
    {
      const int a_b = a.act[b];
      const float* __restrict__ w0 = (st ? a.Pon.wa : a.Pon.wv) + 64 * wv + 4 * g;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (st) {
          for (int j = 0; j < A; ++j) {
            const float cf = (j == a_b ? 1.f : 0.f) - invA;
            const float4 w = *reinterpret_cast<const float4*>(w0 + (int64_t)j * QW_HS + 16 * m);
            s.x = fmaf(cf, w.x, s.x); s.y = fmaf(cf, w.y, s.y); s.z = fmaf(cf, w.z, s.z); s.w = fmaf(cf, w.w, s.w);
          }
        } else {
          s = *reinterpret_cast<const float4*>(w0 + 16 * m);
        }
        u[m][0] = s.x; u[m][1] = s.y; u[m][2] = s.z; u[m][3] = s.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) S[m][i] = 0.f;
      }
    }
    iqw_stage_cos(ka, cword, b, 0, N, Ts, Chi, Clo, nullptr,
                  st == 0 && ka.cosT != nullptr ? ka.cosT + (int64_t)b * N * IQN_E : nullptr, tid);
    const float* __restrict__ gk = a.dhead + (int64_t)b * J;
    for (int t = 0; t < NT; ++t) {
      f32x4 acc[4];
      iqw_pre_tile(f, Chi, Clo, t, N, lane, acc);
      const int k = 16 * t + (lane & 15);
      const bool ok = k < N;
      const float gv = ok ? gk[k] : 0.f;
      float* __restrict__ dp = ka.dpre + ((int64_t)b * N + min(k, N - 1)) * (2 * QW_HS) + c0 + 4 * g;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pre = acc[m][i] + f.be[m][i];
          S[m][i] = fmaf(gv, fmaxf(pre, 0.f), S[m][i]);
          d[i] = pre > 0.f ? (gv * u[m][i]) * h[m][i] : 0.f;
        }
        if (ok) *reinterpret_cast<float4*>(dp + 16 * m) = make_float4(d[0], d[1], d[2], d[3]);
      }
    }
    // S over the 16 samples of a DPP row; the row's first lane stores its four columns
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float dh[4], xg[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float s = row16_sum(S[m][i]);
        xg[i] = h[m][i] * s;
        dh[i] = h[m][i] > 0.f ? u[m][i] * s : 0.f;
      }
      if ((lane & 15) == 0) {
        const int64_t o = (int64_t)b * (2 * QW_HS) + c0 + 16 * m + 4 * g;
        *reinterpret_cast<float4*>(ka.xg + o) = make_float4(xg[0], xg[1], xg[2], xg[3]);
        if (split) {
          uint32_t h0, l0, h1, l1;
          split_pk_bf16_h(dh[0], dh[1], h0, l0);
          split_pk_bf16_h(dh[2], dh[3], h1, l1);
          *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(a.lo.dH + o) = make_uint2(l0, l1);
        } else {
          *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(pack_bf16x2(dh[0], dh[1]), pack_bf16x2(dh[2], dh[3]));
        }
      }
    }
    __syncthreads();                       // the row's cosines are consumed before the next row's are staged
  }
}

// ------------------------------------------------------------------------------------------------ launcher
template <bool RESCALE>
static inline void iqw_finish_launch(const IqnWideArgs& a, hipStream_t st) {
  const int grid = (a.h.io.B + 3) / 4;
  switch ((a.h.N + 63) / 64) {
    case 1: iqn_wide_finish_kernel<RESCALE, 1><<<grid, QW_NT, 0, st>>>(a); break;
    case 2: iqn_wide_finish_kernel<RESCALE, 2><<<grid, QW_NT, 0, st>>>(a); break;
    case 3: iqn_wide_finish_kernel<RESCALE, 3><<<grid, QW_NT, 0, st>>>(a); break;
    default: iqn_wide_finish_kernel<RESCALE, 4><<<grid, QW_NT, 0, st>>>(a); break;
  }
}

static inline void miqn_finish_launch(const MiqnWideArgs& a, hipStream_t st) {
  const int grid = (a.w.h.io.B + 3) / 4;
  switch ((a.w.h.N + 63) / 64) {
    case 1: miqn_wide_finish_kernel<1><<<grid, QW_NT, 0, st>>>(a); break;
    case 2: miqn_wide_finish_kernel<2><<<grid, QW_NT, 0, st>>>(a); break;
    case 3: miqn_wide_finish_kernel<3><<<grid, QW_NT, 0, st>>>(a); break;
    default: miqn_wide_finish_kernel<4><<<grid, QW_NT, 0, st>>>(a); break;
  }
}

// The three launches of either head: `ma` null = the plain row plan and target, else the Munchausen ones.
static int iqw_launch(const IqnWideArgs& wa, const MiqnWideArgs* ma, hipStream_t st) {
  const IqnArgs& a = wa.h;
  if (!qw_head_ok(a.io, a.N, wa.L) || !(a.kappa > 0.f)) return (int)hipErrorInvalidValue;
  if (!iqn_embed_ok(a.Eon) || !iqn_embed_ok(a.Etg)) return (int)hipErrorInvalidValue;
  if (a.ctr == nullptr || a.dpre == nullptr || a.xg == nullptr) return (int)hipErrorInvalidValue;
  // 16-byte stores of dpre, xg and the cosines
  if (((uintptr_t)a.dpre | (uintptr_t)a.xg | (uintptr_t)a.cosT) & 15) return (int)hipErrorInvalidValue;
  const size_t lds = iqw_lds(a.N);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  static bool lds_set = false;             // raised once, to the largest N's: not again inside a captured step
  if (!lds_set) {
    for (const void* fn : {reinterpret_cast<const void*>(iqn_wide_logits_kernel<false>),
                           reinterpret_cast<const void*>(iqn_wide_logits_kernel<true>),
                           reinterpret_cast<const void*>(iqn_wide_bwd_kernel)}) {
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)iqw_lds(256));
      if (e != hipSuccess) return (int)e;
    }
    lds_set = true;
  }
  // one block per CU: half the CUs walk each stream
  const int cap = a.max_blocks > 0 ? a.max_blocks : (iqn_cu_count() + 1) / 2;
  const int B = a.io.B;
  const dim3 lgrid((unsigned)(3 * B < cap ? 3 * B : cap), 2);
  if (ma != nullptr) {
    iqn_wide_logits_kernel<true><<<lgrid, IQW_NT, lds, st>>>(wa);
    miqn_finish_launch(*ma, st);
  } else {
    iqn_wide_logits_kernel<false><<<lgrid, IQW_NT, lds, st>>>(wa);
    if (a.io.rescale_eps > 0.f) iqw_finish_launch<true>(wa, st);
    else iqw_finish_launch<false>(wa, st);
  }
  iqn_wide_bwd_kernel<<<dim3((unsigned)(B < cap ? B : cap), 2), IQW_NT, lds, st>>>(wa);
  APEX_CHECK_LAUNCH();
}

APEX_EXPORT int apex_iqn_wide_head(IqnWideArgs wa, hipStream_t st) { return iqw_launch(wa, nullptr, st); }

APEX_EXPORT int apex_iqn_wide_args_size() { return (int)sizeof(IqnWideArgs); }

// Hon [B] (online S_t), Htg [2B] (target S_t+n, S_t); refuses what apex_iqn_wide_head refuses, a rescaled target, and
// alpha / tau / clip outside the Munchausen target's ranges (csrc/mdqn_head.hip)
APEX_EXPORT int apex_miqn_wide_head(MiqnWideArgs ma, hipStream_t st) {
  if (!(ma.tau > 0.f) || !(ma.clip < 0.f) || !(ma.alpha >= 0.f && ma.alpha <= 1.f)) return (int)hipErrorInvalidValue;
  if (ma.aux == nullptr || ma.w.h.io.rescale_eps != 0.f) return (int)hipErrorInvalidValue;
  return iqw_launch(ma.w, &ma, st);
}

APEX_EXPORT int apex_miqn_wide_args_size() { return (int)sizeof(MiqnWideArgs); }
