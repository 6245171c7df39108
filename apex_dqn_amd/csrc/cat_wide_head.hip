// Wide categorical (C51) and histogram-loss (HL-Gauss) heads: Runtime.dist_head = "categorical" / "hl_gauss" with
// Runtime.wide_atoms, any 2 <= N <= 256 atoms per action.  The definitions are csrc/c51_head.hip's (the softmax, q,
// a* as the first maximum, the projection with its j-sum in increasing j, the HL-Gauss target in fp64 rounded once,
// loss, td_abs, g, dhead [B][(A + 1) N], dH); the head weights, the flat layout and the checkpoint keys are the
// narrow heads'.  Only the mapping changes.
//
// c51_head_kernel / hlg_head_kernel map one lane to one atom and form the logits as fp32 VALU dot products in LDS;
// neither survives N > 64.  Here a head is the three launches of csrc/wide_head.h on one stream:
//
//   qr_wide_logits_kernel   L [3B][Jp] = H . W^T without biases (MFMA, the weights as bf16 hi + lo)
//   cat_wide_finish_kernel  <KIND, RESCALE, NQ> one wave per sample, four per block.  Lane l owns atoms l, l + 64, ..
//                           (NQ = ceil(N / 64) register sets; an atom past N has the logit -3.0e38, p = m = 0 and is
//                           masked out of every max and sum).  Softmax per action: the lane's max over its sets, then
//                           the wave max; expf, the lane's partial over its sets, then the wave sum; p, log p and
//                           the expectation sum_i p_i z_i the same way.
//                             C51: p'_j and b_j of the target row stay in the register sets of their owner lanes; the
//                             j loop runs in increasing j and fetches (p'_j, b_j) with a wave-uniform readlane from
//                             set j / 64.  The triangle of b_j covers atoms floor(b_j) and floor(b_j) + 1 only, so
//                             only the one or two register sets that hold them are updated (a wave-uniform choice;
//                             the sets left out would add +0.0f, which is exact, and no j changes places).
//                             HLG: y from the target expectation of a*, then E = erf((e - y) inv) in fp64.  Bin i's
//                             upper edge and bin i + 1's lower edge are the same fp64 number (csrc/c51_head.hip), so
//                             a lane evaluates the lower edge of each of its bins and takes the upper one from lane
//                             l + 1 -- lane 63 of set s from lane 0 of set s + 1 -- and the upper edge of bin N - 1,
//                             which is E_N, is evaluated once by every lane (wave-uniform): NQ + 1 erf per lane
//                             instead of 2 NQ.  E_0 by readlane.  m_i = fp32((E_i+1 - E_i) / (E_N - E_0)).
//                           Then the S_t pass: q of every action (q_out), the taken action's p and log p, loss = -w
//                           sum_i m_i log p_i, td_abs against sum_i m_i z_i (C51) or y (HLG), the dhead row.  It
//                           carries dist_head_side's duties: the head-gradient region is zeroed by all blocks, the
//                           IsNorm statistic is left by block 0's last wave.
//   qr_wide_dh_kernel       dH [B][1024] = relu'(h) (dhead . W) per stream (MFMA)
//
// The actor side (both kinds: HL-Gauss actors use the C51 actor head) is the logits kernel with one weight set on
// the E env rows and cat_wide_actor_finish_kernel: one wave per row, the expected q per action, then dist_actor_draw
// with c51_actor_head_kernel's counter-RNG words.  Nothing depends on the order blocks run in (no float atomics).
#include <cmath>

#include "wide_head.h"

enum { CW_C51 = 0, CW_HLG = 1 };

// C51Args / HlgArgs / C51ActorArgs (csrc/c51_head.hip, csrc/dist_head.h) with the logits workspace appended
struct C51WideArgs {
  HeadIO io;
  int N;
  float vmin, vmax;
  float* L;             // [3B][Jp] fp32 logits workspace (qr_wide_jp)
};
struct HlgWideArgs {
  HeadIO io;
  int N;
  float vmin, vmax, sigma_ratio;
  float* L;
};
struct C51WideActorArgs {
  ActorIO io;
  int N;
  float vmin, vmax;
  float* L;             // [E][Jp]
};
static_assert(std::is_standard_layout_v<C51WideArgs> && std::is_trivially_copyable_v<C51WideArgs> &&
              std::is_standard_layout_v<HlgWideArgs> && std::is_trivially_copyable_v<HlgWideArgs> &&
              std::is_standard_layout_v<C51WideActorArgs> && std::is_trivially_copyable_v<C51WideActorArgs>);

// ------------------------------------------------------------------------------------------------ finish
// softmax over the atoms of action j of row r: this lane's probabilities and log-probabilities of its NQ atoms (0
// past N); returns the expectation sum_i p_i z_i (wave-uniform)
template <int NQ>
__device__ __forceinline__ float cw_action(const QWRow<NQ>& r, int j, int N, int lane, const float* z, float* p,
                                           float* lp) {
  float l[NQ], mx = -3.0e38f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    l[s] = 64 * s + lane < N ? qw_theta(r, j, s, N, lane) : -3.0e38f;
    mx = fmaxf(mx, l[s]);
  }
  mx = wave_max(mx);
  float es = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    p[s] = 64 * s + lane < N ? expf(l[s] - mx) : 0.f;
    es += p[s];
  }
  const float Z = wave_sum_dpp(es), lZ = logf(Z);
  float pz = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    p[s] = p[s] / Z;
    lp[s] = 64 * s + lane < N ? (l[s] - mx) - lZ : 0.f;
    pz += p[s] * z[s];
  }
  return wave_sum_dpp(pz);
}

// the first maximum of the expected q over the actions of row r (wave-uniform)
template <int NQ>
__device__ __forceinline__ int cw_astar(const QWRow<NQ>& r, int A, int N, int lane, const float* z) {
  float best = -3.4e38f, p[NQ], lp[NQ];
  int astar = 0;
  for (int j = 0; j < A; ++j) {
    const float q = cw_action(r, j, N, lane, z, p, lp);
    if (q > best) { best = q; astar = j; }
  }
  return __builtin_amdgcn_readfirstlane(astar);
}

__device__ __forceinline__ float cw_readlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

template <int KIND, bool RESCALE, int NQ>
__global__ void __launch_bounds__(QW_NT) cat_wide_finish_kernel(HlgWideArgs ka) {
  const HeadIO& a = ka.io;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int B = a.B, A = a.A, N = ka.N, J = (A + 1) * N, Jp = qr_wide_jp(A, N);
  // zero the head-gradient region that the head weight gradient accumulates into
  if (a.zero_ptr != nullptr)
    for (int i = blockIdx.x * QW_NT + tid; i < a.zero_n; i += gridDim.x * QW_NT) a.zero_ptr[i] = 0.f;
  const int b_raw = blockIdx.x * 4 + wv;
  const bool live = b_raw < B;
  const int b = min(b_raw, B - 1);
  const int a_b = a.act[b];
  const float rew = a.rew[b], gam = a.gam[b];
  const float w = a.isw != nullptr ? a.isw[b] : 1.f;
  const float vmin = ka.vmin, vmax = ka.vmax;
  const float delta = (vmax - vmin) / (float)(N - 1);
  float z[NQ], fi[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    fi[s] = (float)(64 * s + lane);
    z[s] = vmin + fi[s] * delta;
  }
  // double DQN: a* from the online net at S_t+n
  const int astar = cw_astar(qw_row<NQ>(ka.L + (int64_t)(B + b) * Jp, a.Pon, A, N, lane), A, N, lane, z);
  // the target row m: register set s of lane l holds m_(64 s + l)
  float m[NQ], y = 0.f;
  {
    float pg[NQ], lpg[NQ];
    const float qg = cw_action(qw_row<NQ>(ka.L + (int64_t)(2 * B + b) * Jp, a.Ptg, A, N, lane), astar, N, lane, z, pg, lpg);
    if constexpr (KIND == CW_C51) {
      // the target net's distribution of a*, projected onto the support
      float bj[NQ];
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        float tz0;
        if constexpr (RESCALE) tz0 = value_rescale_target(rew, gam, z[s], a.rescale_eps);
        else tz0 = rew + gam * z[s];
        bj[s] = (fminf(fmaxf(tz0, vmin), vmax) - vmin) / delta;
        m[s] = 0.f;
      }
#pragma unroll
      for (int sj = 0; sj < NQ; ++sj) {
        const int nj = min(64, N - 64 * sj);
        for (int jj = 0; jj < nj; ++jj) {      // increasing j: the oracle's order
          const float pp = cw_readlane(pg[sj], jj), bb = cw_readlane(bj[sj], jj);
          const int s0 = (int)bb >> 6, s1 = ((int)bb + 1) >> 6;      // the sets of atoms floor(b_j), floor(b_j) + 1
#pragma unroll
          for (int s = 0; s < NQ; ++s)
            if (NQ == 1 || s == s0 || s == s1) m[s] += pp * fmaxf(0.f, 1.f - fabsf(bb - fi[s]));
        }
      }
    } else {
      // the scalar target from the target net's expectation of a*, then its Gaussian mass per bin
      float y0;
      if constexpr (RESCALE) y0 = value_rescale_target(rew, gam, qg, a.rescale_eps);
      else y0 = rew + gam * qg;
      y = fminf(fmaxf(y0, vmin), vmax);
      const double v0 = (double)vmin;
      const double dl = ((double)vmax - v0) / (double)(N - 1);
      const double inv = 1.0 / ((double)ka.sigma_ratio * dl * 1.4142135623730951);
      double El[NQ];        // the lower edge of this lane's bins (a lane past N repeats the last bin)
#pragma unroll
      for (int s = 0; s < NQ; ++s)
        El[s] = erf((v0 + ((double)min(64 * s + lane, N - 1) - 0.5) * dl - (double)y) * inv);
      const double EN = erf((v0 + ((double)(N - 1) + 0.5) * dl - (double)y) * inv);      // wave-uniform
      const double E0 = __shfl(El[0], 0, 64);
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        double up = __shfl(El[s], (lane + 1) & 63, 64);
        if (s + 1 < NQ) {
          const double h0 = __shfl(El[s + 1 < NQ ? s + 1 : s], 0, 64);
          if (lane == 63) up = h0;
        }
        if (64 * s + lane == N - 1) up = EN;
        m[s] = (float)((up - El[s]) / (EN - E0));
      }
    }
#pragma unroll
    for (int s = 0; s < NQ; ++s)
      if (64 * s + lane >= N) m[s] = 0.f;
  }
  // S_t: q of every action, the taken action's distribution
  float p_sa[NQ], lp_sa[NQ], q_sa = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) p_sa[s] = lp_sa[s] = 0.f;
  {
    const QWRow<NQ> rt = qw_row<NQ>(ka.L + (int64_t)b * Jp, a.Pon, A, N, lane);
    float p[NQ], lp[NQ];
    for (int j = 0; j < A; ++j) {
      const float q = cw_action(rt, j, N, lane, z, p, lp);
      if (a.q_out != nullptr && live && lane == 0) a.q_out[(int64_t)b * A + j] = q;
      if (j == a_b) {
        q_sa = q;
#pragma unroll
        for (int s = 0; s < NQ; ++s) { p_sa[s] = p[s]; lp_sa[s] = lp[s]; }
      }
    }
  }
  float cs = 0.f, mz = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    cs += m[s] * lp_sa[s];
    mz += m[s] * z[s];
  }
  const float ce = -wave_sum_dpp(cs);
  float ref;
  if constexpr (KIND == CW_C51) ref = wave_sum_dpp(mz);
  else ref = y;
  if (live && lane == 0) {
    a.td_abs[b] = fabsf(ref - q_sa);
    a.loss[b] = w * ce;
  }
  // the dhead row: d v[i] = g_i, d adv[j, i] = g_i ([j = a_b] - 1 / A)
  if (live) {
    float* __restrict__ dh = a.dhead + (int64_t)b * J;
    const float invA = 1.0f / (float)A;
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const int i = 64 * s + lane;
      if (i >= N) continue;
      const float g = w * (p_sa[s] - m[s]) * a.grad_scale;
      dh[i] = g;
      for (int j = 0; j < A; ++j) dh[N + j * N + i] = g * ((j == a_b ? 1.f : 0.f) - invA);
    }
  }
  // batch-max IS statistic: block 0's last wave
  if ((a.isn.out != nullptr || a.isn.valid_count != nullptr) && blockIdx.x == 0 && wv == QW_NT / 64 - 1)
    head_is_norm(a, lane);
}

// ------------------------------------------------------------------------------------------------ actor
// expected q per action + epsilon-greedy, one wave per env row (four per block; a wave past E repeats the last row
// and stores nothing)
template <int NQ>
__global__ void __launch_bounds__(QW_NT) cat_wide_actor_finish_kernel(C51WideActorArgs ka) {
  const ActorIO& a = ka.io;
  const int lane = threadIdx.x & 63;
  const int A = a.A, N = ka.N;
  const int e_raw = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = e_raw < a.E;
  const int e = min(e_raw, a.E - 1);
  const float delta = (ka.vmax - ka.vmin) / (float)(N - 1);
  float z[NQ], p[NQ], lp[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) z[s] = ka.vmin + (float)(64 * s + lane) * delta;
  const QWRow<NQ> r = qw_row<NQ>(ka.L + (int64_t)e * qr_wide_jp(A, N), a.P, A, N, lane);
  int best = 0;
  float bq = -3.4e38f;
  for (int j = 0; j < A; ++j) {
    const float q = cw_action(r, j, N, lane, z, p, lp);
    if (q > bq) { bq = q; best = j; }
    if (live && lane == 0) a.q_out[(int64_t)e * A + j] = q;
  }
  if (live && lane == 0) dist_actor_draw(best, e, A, a.eps, a.seed, a.ctr, a.a_out);
}

// ------------------------------------------------------------------------------------------------ launchers
template <int KIND, bool RESCALE>
static inline void cw_finish_launch(const HlgWideArgs& a, hipStream_t st) {
  const int grid = (a.io.B + 3) / 4;
  switch ((a.N + 63) / 64) {
    case 1: cat_wide_finish_kernel<KIND, RESCALE, 1><<<grid, QW_NT, 0, st>>>(a); break;
    case 2: cat_wide_finish_kernel<KIND, RESCALE, 2><<<grid, QW_NT, 0, st>>>(a); break;
    case 3: cat_wide_finish_kernel<KIND, RESCALE, 3><<<grid, QW_NT, 0, st>>>(a); break;
    default: cat_wide_finish_kernel<KIND, RESCALE, 4><<<grid, QW_NT, 0, st>>>(a); break;
  }
}

// logits -> finish -> dH on one stream; `a` has passed the launcher's checks
template <int KIND>
static inline int cw_head_launch(const HlgWideArgs& a, hipStream_t st) {
  qw_launch_head_logits(a.io, a.N, a.L, st);
  if (a.io.rescale_eps > 0.f) cw_finish_launch<KIND, true>(a, st);
  else cw_finish_launch<KIND, false>(a, st);
  qw_launch_dh(a.io, a.N, st);
  APEX_CHECK_LAUNCH();
}

APEX_EXPORT int apex_c51_wide_head(C51WideArgs a, hipStream_t st) {
  if (!qw_head_ok(a.io, a.N, a.L) || !(a.vmin < a.vmax)) return (int)hipErrorInvalidValue;
  HlgWideArgs k;
  k.io = a.io; k.N = a.N; k.vmin = a.vmin; k.vmax = a.vmax; k.sigma_ratio = 0.f; k.L = a.L;
  return cw_head_launch<CW_C51>(k, st);
}

APEX_EXPORT int apex_hlg_wide_head(HlgWideArgs a, hipStream_t st) {
  if (!qw_head_ok(a.io, a.N, a.L) || !(a.vmin < a.vmax) || !(a.sigma_ratio > 0.f) || !std::isfinite(a.sigma_ratio))
    return (int)hipErrorInvalidValue;
  return cw_head_launch<CW_HLG>(a, st);
}

static inline void cw_actor_finish_launch(const C51WideActorArgs& a, hipStream_t st) {
  const int grid = (a.io.E + 3) / 4;
  switch ((a.N + 63) / 64) {
    case 1: cat_wide_actor_finish_kernel<1><<<grid, QW_NT, 0, st>>>(a); break;
    case 2: cat_wide_actor_finish_kernel<2><<<grid, QW_NT, 0, st>>>(a); break;
    case 3: cat_wide_actor_finish_kernel<3><<<grid, QW_NT, 0, st>>>(a); break;
    default: cat_wide_actor_finish_kernel<4><<<grid, QW_NT, 0, st>>>(a); break;
  }
}

APEX_EXPORT int apex_c51_wide_actor_head(C51WideActorArgs a, hipStream_t st) {
  const ActorIO& io = a.io;
  if (!qw_actor_ok(io, a.N, a.L) || !(a.vmin < a.vmax)) return (int)hipErrorInvalidValue;
  qw_launch_actor_logits(io, a.N, a.L, st);
  cw_actor_finish_launch(a, st);
  APEX_CHECK_LAUNCH();
}

// The finish alone, on logits the caller has written into L (csrc/noisy_actor.hip noisy_env_logits_kernel: the
// per-env noisy logits; io.P then carries the mu biases, io.H is not read)
APEX_EXPORT int apex_c51_wide_actor_finish(C51WideActorArgs a, hipStream_t st) {
  if (!qw_actor_ok(a.io, a.N, a.L) || !(a.vmin < a.vmax)) return (int)hipErrorInvalidValue;
  cw_actor_finish_launch(a, st);
  APEX_CHECK_LAUNCH();
}

// sizeof the three argument blocks (which = 0 / 1 / 2) for the ctypes mirrors
APEX_EXPORT int apex_cat_wide_args_size(int which) {
  return which == 0 ? (int)sizeof(C51WideArgs) : which == 1 ? (int)sizeof(HlgWideArgs) : (int)sizeof(C51WideActorArgs);
}
