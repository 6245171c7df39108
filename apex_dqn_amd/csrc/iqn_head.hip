// Implicit quantile (IQN) dueling head for the NatureCNN learner and actors (Dabney et al. 2018).
//
// Head weights at the SCALAR head's shapes: wv [HS], bv [1], wa [A][HS], ba [A]; HS = 512.  The
// embedding We [2 HS][64], be [2 HS] gates the stream activations h = [hv | ha] of one state:
//
//   c_i(tau)   = cos(pi i tau), i = 0..63        pre(tau) = We c(tau) + be      phi = relu(pre)
//   x(tau)     = h * phi(tau)
//   v(tau)     = wv . x[:HS] + bv                adv_a(tau) = wa[a] . x[HS:] + ba[a]
//   theta[a]   = v + adv_a - mean_a' adv_a'      q[a] = mean over the samples of theta[a]
//
// Every fraction is tau = apex_uniform(seed_q, c, idx) (learner/iqn.py is the host mirror):
//   learner:  c = 64 u (u = ctr - base, read here), idx = (3 b + set) 64 + k, N fractions per
//             set: set 0 the online net at S_t, 1 the online net at S_t+n (a* = first maximum
//             of its mean), 2 the target net at S_t+n (T_j = R + G theta_target[a*](tau'_j))
//   actors:   c = 64 t + stream (t = tau_ctr[0]), idx = e 64 + k; or tau_k = (2 k + 1) / (2 K)
// The loss, g, td_abs and dhead [B][(A + 1) N] are csrc/qr_head.hip's with tau_i of set 0 in
// the place of the midpoints (lane = sample).
//
// iqn_head_kernel: a persistent grid of 512-thread blocks walks the batch DIST_SPB samples at
// a time.  Thread t owns value column t and advantage column HS + t and keeps their two We
// rows in registers.  Per staged activation row (target rows first, then the online ones: two
// weight loads per walk step, a third for the backward): the N cosine vectors go to LDS, every thread
// forms pre / phi / x of its two columns (broadcast ds_read_b128 of the cosines) and the
// (A + 1) N logits are reduced over the columns: a DPP wave sum per (row a', sample k), the
// eight wave partials added through LDS in wave order.  Wave s then finishes sample s as
// qr_head_kernel does.  The backward recomputes phi of set 0 and writes, per sample,
//   dH    [2 HS]     = [h > 0] sum_k phi_k dx_k      dx_k = g_k wv (value) / g_k sum_a coef_a wa[a]
//   dpre  [N][2 HS]  = [pre_k > 0] dx_k h            coef_a = [a = a_b] - 1/A
//   xg    [2 HS]     = sum_k g_k h phi_k             gsum = sum_k g_k          cos [N][64]
// for iqn_wgrad_prio_kernel (csrc/iqn_wgrad.h, launched from csrc/sumtree.hip beside the priority write-back),
// whose sums over the batch all run in a fixed order (no float atomics):
//   G[wv] = sum_b xg_b[:HS]      G[wa][a] = sum_b coef_a(b) xg_b[HS:]     G[bv], G[ba] from gsum
//   G[btau] = sum_{b,k} dpre     G[wtau] = sum_{b,k} dpre (x) cos         (waves and eight blocks split b k;
//                                                                          a small second launch adds the partials)
//
// iqn_actor_head_kernel: one block per env row, the same logits, q = mean over the K samples
// and the epsilon-greedy draw of actor_head_kernel (same counter-RNG words).
#include "iqn_wgrad.h"     // (IQN_E, IqnEmbed, IqnActorArgs; the weight-gradient body lives there)

struct IqnArgs {
  HeadIO io;            // Hon [2B], Htg [B]; dhead [B][(A + 1) N]
  IqnEmbed Eon, Etg;    // (right behind io: with them after `base` iqn_head_kernel measured 0.5 % slower at A = 4)
  int N;
  float kappa;
  uint64_t seed_q;
  const int64_t* ctr;   // draw counter; u = ctr - base
  const int64_t* base;  // null: 0
  float* tau_out;       // [B][3][N] or null
  float* dpre;          // [B][N][2 HS]
  float* cosT;          // [B][N][64]
  float* xg;            // [B][2 HS]
  float* gsum;          // [B]
  int max_blocks;       // <= 0: the CU count
};
static_assert(std::is_standard_layout_v<IqnArgs> && std::is_trivially_copyable_v<IqnArgs>);

// cos(pi i tau): the fp32 product i tau rounds; its exact residual (one fma) enters to first order
__device__ __forceinline__ float iqn_cos(int i, float tau) {
  const float fi = (float)i;
  const float p = __fmul_rn(fi, tau);
  const float r = fmaf(fi, tau, -p);
  return fmaf(-3.14159265358979323846f * r, sinpif(p), cospif(p));
}

__device__ __forceinline__ void iqn_load_we(const IqnEmbed& E, int tid, float* wev, float* wea, float& bev, float& bea) {
  const float4* pv = reinterpret_cast<const float4*>(E.w + (int64_t)tid * IQN_E);
  const float4* pa = reinterpret_cast<const float4*>(E.w + (int64_t)(DIST_HS + tid) * IQN_E);
#pragma unroll
  for (int q = 0; q < IQN_E / 4; ++q) {
    const float4 x = pv[q], y = pa[q];
    wev[4 * q] = x.x; wev[4 * q + 1] = x.y; wev[4 * q + 2] = x.z; wev[4 * q + 3] = x.w;
    wea[4 * q] = y.x; wea[4 * q + 1] = y.y; wea[4 * q + 2] = y.z; wea[4 * q + 3] = y.w;
  }
  bev = E.b[tid];
  bea = E.b[DIST_HS + tid];
}

// pre of this thread's two columns at the cosine vector cs [64] (LDS, the same address in every lane)
__device__ __forceinline__ void iqn_pre(const float* wev, const float* wea, float bev, float bea, const float* cs,
                                        float& pv, float& pa) {
  pv = bev;
  pa = bea;
#pragma unroll
  for (int q = 0; q < IQN_E / 4; ++q) {
    const float4 c = *reinterpret_cast<const float4*>(cs + 4 * q);
    pv = fmaf(wev[4 * q], c.x, pv); pv = fmaf(wev[4 * q + 1], c.y, pv);
    pv = fmaf(wev[4 * q + 2], c.z, pv); pv = fmaf(wev[4 * q + 3], c.w, pv);
    pa = fmaf(wea[4 * q], c.x, pa); pa = fmaf(wea[4 * q + 1], c.y, pa);
    pa = fmaf(wea[4 * q + 2], c.z, pa); pa = fmaf(wea[4 * q + 3], c.w, pa);
    // at most four cosine reads in flight: all sixteen beside the weights went to scratch
    if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
  }
}

// the N cosine vectors of the fractions ts [N] -> cs [N][64] (and to `out`, or null)
__device__ __forceinline__ void iqn_fill_cos(const float* ts, int N, float* cs, float* out, int tid) {
  for (int idx = tid; idx < N * IQN_E; idx += DIST_NT) {
    const float c = iqn_cos(idx & (IQN_E - 1), ts[idx >> 6]);
    cs[idx] = c;
    if (out != nullptr) out[idx] = c;
  }
}

// One activation row's logits (no biases) -> L [Jp]: column a' N + k (a' = 0 the value row, 1 + a action a).
// hv / ha: this thread's two activations; cs [N][64] the row's cosines; Pw [8][Jp] wave partials.
// Contains two block barriers; the caller barriers before cs / Pw / L are written again.
// PRE (the actor head at A <= 8): the head weights of this thread's columns are loaded once per row, ahead of
// the sample loop; else the next action's weight is in flight while this action's wave sum runs.
template <bool PRE>
__device__ __forceinline__ void iqn_row_logits(const float* wev, const float* wea, float bev, float bea,
                                               const HeadParams& P, float hv, float ha, const float* cs, int A, int N,
                                               int Jp, float* Pw, float* L, int tid, int lane, int wv) {
  float* pw = Pw + wv * Jp;
  const float wvc = P.wv[tid];
  float wr[8];
  if constexpr (PRE) {
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[j] = j < A ? P.wa[j * DIST_HS + tid] : 0.f;
  }
#pragma unroll 1
  for (int k = 0; k < N; ++k) {
    float pv, pa;
    iqn_pre(wev, wea, bev, bea, cs + k * IQN_E, pv, pa);
    const float xv = hv * fmaxf(pv, 0.f), xa = ha * fmaxf(pa, 0.f);
    const float sv = wave_sum_dpp(wvc * xv);
    if (lane == 0) pw[k] = sv;
    if constexpr (PRE) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < A) {
          const float sa = wave_sum_dpp(wr[j] * xa);
          if (lane == 0) pw[(1 + j) * N + k] = sa;
        }
      }
    } else {
      float wn = P.wa[tid];
      for (int j = 0; j < A; ++j) {
        const float w = wn;
        wn = P.wa[min(j + 1, A - 1) * DIST_HS + tid];
        const float sa = wave_sum_dpp(w * xa);
        if (lane == 0) pw[(1 + j) * N + k] = sa;
      }
    }
  }
  __syncthreads();
  const int J = (A + 1) * N;
  for (int j = tid; j < J; j += DIST_NT) {
    float s = Pw[j];
#pragma unroll
    for (int w = 1; w < DIST_NT / 64; ++w) s += Pw[w * Jp + j];
    L[j] = s;
  }
  __syncthreads();
}

// One row's dueling terms, lane = sample: L = the logits without biases
struct IqnRow {
  const float* L;
  const float* ba;
  float v, mean;
};

__device__ __forceinline__ IqnRow iqn_row(const float* L, const HeadParams& P, int A, int N, int lane) {
  IqnRow r;
  r.L = L;
  r.ba = P.ba;
  const bool valid = lane < N;
  r.v = valid ? L[lane] + P.bv[0] : 0.f;
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += valid ? L[N + a * N + lane] + P.ba[a] : 0.f;
  r.mean = s / (float)A;
  return r;
}

__device__ __forceinline__ float iqn_theta(const IqnRow& r, int a, int N, int lane) {
  return lane < N ? r.v + (r.L[N + a * N + lane] + r.ba[a]) - r.mean : 0.f;
}

static inline size_t iqn_head_lds(int A, int N) {
  const int J = (A + 1) * N, Jp = (J + 3) & ~3;
  return (size_t)(3 * DIST_SPB * (2 * DIST_HS + Jp + 64) + (DIST_NT / 64) * Jp + DIST_SPB * N * IQN_E) * sizeof(float);
}

// RESCALE (Runtime.value_rescale): T_j = h(R + G h^-1(theta_target[a*, j])) per target sample (csrc/value_rescale.h)
// and td_abs from the mean of the transformed T_j summed in increasing j, as qr_head_kernel<true>.
template <bool RESCALE>
__global__ void __launch_bounds__(DIST_NT) iqn_head_kernel(IqnArgs ka) {
  const HeadIO& a = ka.io;
  extern __shared__ __attribute__((aligned(16))) float iqn_smem[];
  constexpr int HS = DIST_HS, ROW = 2 * HS, SPB = DIST_SPB, NR = 3 * SPB, NW = DIST_NT / 64;
  const int tid0 = threadIdx.x;
  const int B = a.B, A = a.A, N = ka.N, J = (A + 1) * N;
  const int Jp = (J + 3) & ~3;
  float* Hs = iqn_smem;                    // [NR][ROW]: rows s (S_t), SPB + s (online S_t+n), 2 SPB + s (target)
  float* Ls = Hs + NR * ROW;               // [NR][Jp] logits (no biases); rows s later hold the dhead rows
  float* Pw = Ls + NR * Jp;                // [NW][Jp] wave partials of the row in flight
  float* Cs = Pw + NW * Jp;                // [SPB][N][64] cosines: slot s holds the last row of sample s (set 0 at the end)
  float* Ts = Cs + SPB * N * IQN_E;        // [NR][64] fractions
  const bool split = a.lo.Hon != nullptr;

  dist_head_side(a, tid0, tid0 & 63, tid0 >> 6);
  int64_t u = ka.ctr[0] - (ka.base != nullptr ? ka.base[0] : 0);
  u = u < 0 ? 0 : u;
  const uint64_t cword = 64ull * (uint64_t)u;
  const float invA = 1.0f / (float)A;

  const int npairs = (B + SPB - 1) / SPB;
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int b0 = pair * SPB;
    // the thread index is re-read per pair: per-thread addresses are then formed where they are used and
    // not kept live across the walk beside the 128 weight registers (that spilled to scratch)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wv = tid >> 6;
    __syncthreads();                       // the previous pair's LDS is consumed
    dist_head_stage(a, Hs, b0, tid, split);
    if (tid < NR * 64) {
      const int r = tid >> 6, k = tid & 63;
      const int s = r % SPB, set = r / SPB;
      const int b = min(b0 + s, B - 1);
      float tau = 0.f;
      if (k < N) {
        tau = apex_uniform(ka.seed_q, cword, (uint64_t)(3 * b + set) * 64ull + (uint64_t)k);
        if (ka.tau_out != nullptr && b0 + s < B) ka.tau_out[((int64_t)b * 3 + set) * N + k] = tau;
      }
      Ts[r * 64 + k] = tau;
    }
    float wev[IQN_E], wea[IQN_E], bev, bea;
    // the target rows, then the online rows of S_t+n and of S_t
    auto do_row = [&](int r, const HeadParams& P) {
      const int s = r % SPB;
      __syncthreads();                     // Ts staged; slot s and Pw free
      const bool keep = r < SPB && b0 + s < B && ka.cosT != nullptr;
      iqn_fill_cos(Ts + r * 64, N, Cs + s * N * IQN_E, keep ? ka.cosT + (int64_t)(b0 + s) * N * IQN_E : nullptr, tid);
      __syncthreads();
      // (the PRE form beside this kernel's other live values left 17 registers in scratch)
      iqn_row_logits<false>(wev, wea, bev, bea, P, Hs[r * ROW + tid], Hs[r * ROW + HS + tid], Cs + s * N * IQN_E, A, N,
                            Jp, Pw, Ls + r * Jp, tid, lane, wv);
    };
    __syncthreads();                       // (also keeps the 128 weight loads out of the staging code)
    iqn_load_we(ka.Etg, tid, wev, wea, bev, bea);
#pragma unroll 1
    for (int r = 2 * SPB; r < NR; ++r) do_row(r, a.Ptg);
    iqn_load_we(ka.Eon, tid, wev, wea, bev, bea);
#pragma unroll 1
    for (int ri = 0; ri < 2 * SPB; ++ri) do_row(ri < SPB ? SPB + ri : ri - SPB, a.Pon);

    // ---- wave s finishes sample s (lane = sample), as qr_head_kernel with the drawn fractions
    if (wv < SPB) {
      const int s = wv;
      const bool live = b0 + s < B;
      const int b = min(b0 + s, B - 1);
      const bool valid = lane < N;
      const float invN = 1.0f / (float)N;
      const int a_b = a.act[b];
      const float rew_b = a.rew[b], gam_b = a.gam[b];
      const float w_b = a.isw != nullptr ? a.isw[b] : 1.f;
      const float kappa = ka.kappa;
      int astar = 0;
      {
        const IqnRow rn = iqn_row(Ls + (SPB + s) * Jp, a.Pon, A, N, lane);
        float best = -3.4e38f;
        for (int j = 0; j < A; ++j) {
          const float q = wave_sum_dpp(iqn_theta(rn, j, N, lane)) * invN;
          if (q > best) { best = q; astar = j; }
        }
        astar = __builtin_amdgcn_readfirstlane(astar);
      }
      float T;
      {
        const IqnRow rg = iqn_row(Ls + (2 * SPB + s) * Jp, a.Ptg, A, N, lane);
        if constexpr (RESCALE)
          T = valid ? value_rescale_target(rew_b, gam_b, iqn_theta(rg, astar, N, lane), a.rescale_eps) : 0.f;
        else
          T = valid ? rew_b + gam_b * iqn_theta(rg, astar, N, lane) : 0.f;
      }
      float th_sa = 0.f, q_sa = 0.f;
      {
        const IqnRow rt = iqn_row(Ls + s * Jp, a.Pon, A, N, lane);
        for (int j = 0; j < A; ++j) {
          const float th = iqn_theta(rt, j, N, lane);
          const float q = wave_sum_dpp(th) * invN;
          if (a.q_out != nullptr && live && lane == 0) a.q_out[(int64_t)b * A + j] = q;
          if (j == a_b) { th_sa = th; q_sa = q; }
        }
      }
      const float tau = Ts[s * 64 + lane];
      float rho = 0.f, c = 0.f;
      float tsum = 0.f;                    // RESCALE: sum_j T_j in increasing j (the oracle's order)
      for (int j = 0; j < N; ++j) {
        const float Tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T), j));
        if constexpr (RESCALE) tsum += Tj;
        const float uu = Tj - th_sa;
        const float au = fabsf(uu);
        const float wgt = fabsf(tau - (uu < 0.f ? 1.f : 0.f));
        rho += wgt * (au <= kappa ? 0.5f * uu * uu : kappa * (au - 0.5f * kappa));
        c += wgt * fminf(fmaxf(uu, -kappa), kappa);
      }
      const float sc = invN / kappa;
      const float ls = wave_sum_dpp(valid ? rho * sc : 0.f);
      float et;
      if constexpr (RESCALE) et = tsum * invN;
      else et = wave_sum_dpp(T) * invN;
      const float g = valid ? -w_b * a.grad_scale * (c * sc) : 0.f;
      const float gs = wave_sum_dpp(g);
      if (live && lane == 0) {
        a.td_abs[b] = fabsf(et - q_sa);
        a.loss[b] = w_b * ls;
        if (ka.gsum != nullptr) ka.gsum[b] = gs;
      }
      dist_head_store_dhead(g, live, valid, a_b, A, N, lane, Ls + s * Jp, a.dhead + (int64_t)b * J);
    }
    __syncthreads();

    // ---- backward of set 0 (slot s holds the cosines of set 0).  The online We is loaded again: kept
    // live across wave s's finish above it cost 7 registers of scratch; the second read is an L2 hit
    iqn_load_we(ka.Eon, tid, wev, wea, bev, bea);
#pragma unroll 1
    for (int s = 0; s < SPB; ++s) {
      if (b0 + s >= B) break;
      const int b = b0 + s;
      const int a_b = a.act[b];
      const float* D = Ls + s * Jp;
      const float wvc = a.Pon.wv[tid];
      float weff = 0.f;
      for (int j = 0; j < A; ++j) weff = fmaf((j == a_b ? 1.f : 0.f) - invA, a.Pon.wa[j * HS + tid], weff);
      const float hv = Hs[s * ROW + tid], ha = Hs[s * ROW + HS + tid];
      float dhv = 0.f, dha = 0.f, xgv = 0.f, xga = 0.f;
      float* dp = ka.dpre + (int64_t)b * N * ROW;
#pragma unroll 1
      for (int k = 0; k < N; ++k) {
        const float g = D[k];
        float pv, pa;
        iqn_pre(wev, wea, bev, bea, Cs + (s * N + k) * IQN_E, pv, pa);
        const float fv = fmaxf(pv, 0.f), fa = fmaxf(pa, 0.f);
        const float dxv = g * wvc, dxa = g * weff;
        dhv = fmaf(fv, dxv, dhv);
        dha = fmaf(fa, dxa, dha);
        dp[k * ROW + tid] = pv > 0.f ? dxv * hv : 0.f;
        dp[k * ROW + HS + tid] = pa > 0.f ? dxa * ha : 0.f;
        xgv = fmaf(g, hv * fv, xgv);
        xga = fmaf(g, ha * fa, xga);
      }
      ka.xg[(int64_t)b * ROW + tid] = xgv;
      ka.xg[(int64_t)b * ROW + HS + tid] = xga;
      const float mv = hv > 0.f ? dhv : 0.f, ma = ha > 0.f ? dha : 0.f;
      const bf16_t hv16 = f32_to_bf16(mv), ha16 = f32_to_bf16(ma);
      a.dH[(int64_t)b * ROW + tid] = hv16;
      a.dH[(int64_t)b * ROW + HS + tid] = ha16;
      if (split) {
        a.lo.dH[(int64_t)b * ROW + tid] = f32_to_bf16(mv - bf16_to_f32(hv16));
        a.lo.dH[(int64_t)b * ROW + HS + tid] = f32_to_bf16(ma - bf16_to_f32(ha16));
      }
    }
  }
}

static inline bool iqn_embed_ok(const IqnEmbed& E) {
  return E.w != nullptr && E.b != nullptr && ((uintptr_t)E.w & 15) == 0;
}

static int iqn_cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n < 1)
      n = 256;
    cus = n;
  }
  return cus;
}

APEX_EXPORT int apex_iqn_head(IqnArgs a, hipStream_t st) {
  if (!head_io_ok(a.io) || a.N < 2 || a.N > 64 || a.io.hidden != DIST_HS || !(a.kappa > 0.f))
    return (int)hipErrorInvalidValue;
  if (!iqn_embed_ok(a.Eon) || !iqn_embed_ok(a.Etg)) return (int)hipErrorInvalidValue;
  if (a.ctr == nullptr || a.dpre == nullptr || a.xg == nullptr) return (int)hipErrorInvalidValue;
  const bool rs = a.io.rescale_eps > 0.f;
  const size_t lds = iqn_head_lds(a.io.A, a.N);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  static size_t lds_set[2] = {64 * 1024, 64 * 1024};   // raised once per size and variant: not again inside a captured step
  if (lds > lds_set[rs]) {
    const void* fn = rs ? reinterpret_cast<const void*>(iqn_head_kernel<true>)
                        : reinterpret_cast<const void*>(iqn_head_kernel<false>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    lds_set[rs] = lds;
  }
  const int npairs = (a.io.B + DIST_SPB - 1) / DIST_SPB;
  const int cap = a.max_blocks > 0 ? a.max_blocks : iqn_cu_count();
  const int grid = npairs < cap ? npairs : cap;
  if (rs) iqn_head_kernel<true><<<grid, DIST_NT, lds, st>>>(a);
  else iqn_head_kernel<false><<<grid, DIST_NT, lds, st>>>(a);
  APEX_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ actors
static inline size_t iqn_actor_lds(int A, int K) {
  const int J = (A + 1) * K, Jp = (J + 3) & ~3;
  return (size_t)((1 + DIST_NT / 64) * Jp + K * IQN_E + 64) * sizeof(float);
}

__global__ void __launch_bounds__(DIST_NT) iqn_actor_head_kernel(IqnActorArgs ka) {
  const ActorIO& a = ka.io;
  extern __shared__ __attribute__((aligned(16))) float iqn_smem[];
  constexpr int HS = DIST_HS, ROW = 2 * HS, NW = DIST_NT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int A = a.A, K = ka.K, J = (A + 1) * K, Jp = (J + 3) & ~3;
  float* L = iqn_smem;               // [Jp]
  float* Pw = L + Jp;                // [NW][Jp]
  float* Cs = Pw + NW * Jp;          // [K][64]
  float* Ts = Cs + K * IQN_E;        // [64]
  const int e = blockIdx.x;
  if (tid < 64) {
    float tau = 0.f;
    if (tid < K) {
      if (ka.midpoint) tau = (2.f * (float)tid + 1.f) / (2.f * (float)K);
      else tau = apex_uniform(ka.seed_q, 64ull * (uint64_t)ka.tau_ctr[0] + (uint64_t)ka.stream, (uint64_t)e * 64ull + (uint64_t)tid);
      if (ka.tau_out != nullptr) ka.tau_out[(int64_t)e * K + tid] = tau;
    }
    Ts[tid] = tau;
  }
  float hv = bf16_to_f32(a.H[(int64_t)e * ROW + tid]), ha = bf16_to_f32(a.H[(int64_t)e * ROW + HS + tid]);
  if (a.H_lo != nullptr) {
    hv += bf16_to_f32(a.H_lo[(int64_t)e * ROW + tid]);
    ha += bf16_to_f32(a.H_lo[(int64_t)e * ROW + HS + tid]);
  }
  float wev[IQN_E], wea[IQN_E], bev, bea;
  iqn_load_we(ka.Em, tid, wev, wea, bev, bea);
  __syncthreads();
  iqn_fill_cos(Ts, K, Cs, nullptr, tid);
  __syncthreads();
  if (A <= 8) iqn_row_logits<true>(wev, wea, bev, bea, a.P, hv, ha, Cs, A, K, Jp, Pw, L, tid, lane, wv);
  else iqn_row_logits<false>(wev, wea, bev, bea, a.P, hv, ha, Cs, A, K, Jp, Pw, L, tid, lane, wv);
  if (wv != 0) return;
  const float invK = 1.0f / (float)K;
  const IqnRow r = iqn_row(L, a.P, A, K, lane);
  int best = 0;
  float bq = -3.4e38f;
  for (int j = 0; j < A; ++j) {
    const float q = wave_sum_dpp(iqn_theta(r, j, K, lane)) * invK;
    if (q > bq) { bq = q; best = j; }
    if (lane == 0) a.q_out[(int64_t)e * A + j] = q;
  }
  if (lane == 0) dist_actor_draw(best, e, A, a.eps, a.seed, a.ctr, a.a_out);
}

APEX_EXPORT int apex_iqn_actor_head(IqnActorArgs ka, hipStream_t st) {
  const ActorIO& a = ka.io;
  if (!actor_io_ok(a) || ka.K < 1 || ka.K > 64 || a.hidden != DIST_HS || !iqn_embed_ok(ka.Em) ||
      (!ka.midpoint && ka.tau_ctr == nullptr))
    return (int)hipErrorInvalidValue;
  const size_t lds = iqn_actor_lds(a.A, ka.K);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  static size_t lds_set = 64 * 1024;      // raised once per size: not again inside a captured step
  if (lds > lds_set) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(iqn_actor_head_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    lds_set = lds;
  }
  iqn_actor_head_kernel<<<a.E, DIST_NT, lds, st>>>(ka);
  APEX_CHECK_LAUNCH();
}
