// Distributional (C51) dueling head for the NatureCNN learner: the counterpart of
// csrc/ddqn_head.hip for Runtime.num_atoms = N >= 2 (one lane per atom, N <= 64).
//
// Head weights (fp32, as the scalar head reads them): wv [N][HS], bv [N], wa [A N][HS]
// (row a N + i = action a, atom i), ba [A N]; HS = 512.  Support z_i = v_min + i delta.
//
//   logits   l[a,i] = v[i] + adv[a,i] - mean_a' adv[a',i]      (dueling mean per atom)
//   p[a,.]   = softmax_i l[a,.] (fp32, max-subtracted),  q[a] = sum_i p[a,i] z_i
//   a*       = argmax_a q_online(S_t+n) (first maximum),  p' = p_target(S_t+n)[a*]
//   m_i      = sum_j p'_j max(0, 1 - |b_j - i|),  b_j = (clamp(R + G z_j) - v_min) / delta,
//              summed in increasing j (a gather: no scatter, no atomics)
//   loss_b   = -w_b sum_i m_i log p(S_t)[a_b,i],  td_abs_b = |sum_i m_i z_i - q(S_t)[a_b]|
//   g_i      = w_b (p(S_t)[a_b,i] - m_i) grad_scale;  d v[i] = g_i,
//              d adv[a,i] = g_i ([a = a_b] - 1/A)  -> dhead [B][(A + 1) N]
//   dH       = dhead . W, masked by the stream ReLUs (bf16, or hi / lo planes)
// Runtime.value_rescale (c51_head_kernel<true>, HeadIO.rescale_eps > 0): the support and v_min / v_max live in
// transformed space, b_j = (clamp(h(R + G h^-1(z_j))) - v_min) / delta (csrc/value_rescale.h); the projection and
// td_abs are as above.
//
// c51_head_kernel: one block of DIST_NT threads per DIST_SPB samples, run by csrc/dist_head.h's
// dist_head_frame (staging the activation rows, the logits, the sample's batch row, the dhead
// row and dH: shared with the quantile head, csrc/qr_head.hip).  The kernel hands the frame
// its phase 2, per sample with lane = atom: a* (c51_astar), the projection (p'_j and b_j by
// lane shuffles), then the S_t pass (c51_st_pass: softmax per action, expectations, loss,
// priority, g).  hlg_head_kernel below shares both helpers and differs in the target row.
// Nothing depends on the order blocks run in (no float atomics).
//
// c51_actor_head_kernel: one wave per env row, the logits as in phase 1 with the row in
// registers, then the expected q per action and the epsilon-greedy draw of
// actor_head_kernel (same counter-RNG words).
#include "dist_head.h"

struct C51Args {
  HeadIO io;            // Hon [2B], Htg [B]; q_out the expected q(S_t); dhead [B][(A + 1) N]
  int N;
  float vmin, vmax;
};
static_assert(std::is_standard_layout_v<C51Args> && std::is_trivially_copyable_v<C51Args>);

// softmax over the atoms of action a: this lane's probability and log-probability;
// returns the expectation sum_i p_i z_i (wave-uniform)
__device__ __forceinline__ float c51_action(const DistRow& r, int a, int N, int lane, float z, float& p, float& lp) {
  const bool valid = lane < N;
  const float l = valid ? r.v + (r.L[N + a * N + lane] + r.ba[a * N + lane]) - r.mean : -3.0e38f;
  const float mx = wave_max(l);
  const float e = valid ? expf(l - mx) : 0.f;
  const float Z = wave_sum_dpp(e);
  p = e / Z;
  lp = valid ? (l - mx) - logf(Z) : 0.f;
  return wave_sum_dpp(p * z);
}

// double DQN: a* = the first maximum of the expected q over the actions of logits row L (wave-uniform)
__device__ __forceinline__ int c51_astar(const float* L, const HeadParams& P, int A, int N, int lane, float z) {
  const DistRow rn = dist_row(L, P, A, N, lane);
  float best = -3.4e38f, p, lp;
  int astar = 0;
  for (int j = 0; j < A; ++j) {
    const float q = c51_action(rn, j, N, lane, z, p, lp);
    if (q > best) { best = q; astar = j; }
  }
  return __builtin_amdgcn_readfirstlane(astar);
}

// The S_t pass of both categorical heads against the target row m (this lane's mass): the expected q of every
// action (q_out), the taken action's distribution, loss = -w sum_i m_i log p_i and td_abs = |ref - q[a_b]|
// (ref(): sum_i m_i z_i for C51, y for HL-Gauss; a callable so that C51's wave sum stands beside the loss's and
// the two reductions share packed adds); returns this lane's g.
template <class Ref>
__device__ __forceinline__ float c51_st_pass(const HeadIO& a, const DistSample& d, const float* L, int N, int lane,
                                             float z, float m, Ref ref) {
  const int A = a.A;
  float p, lp, p_sa = 0.f, lp_sa = 0.f, q_sa = 0.f;
  const DistRow rt = dist_row(L, a.Pon, A, N, lane);
  for (int j = 0; j < A; ++j) {
    const float q = c51_action(rt, j, N, lane, z, p, lp);
    if (a.q_out != nullptr && d.live && lane == 0) a.q_out[(int64_t)d.b * A + j] = q;
    if (j == d.a_b) { p_sa = p; lp_sa = lp; q_sa = q; }
  }
  const float ce = -wave_sum_dpp(m * lp_sa);
  const float r = ref();
  if (d.live && lane == 0) {
    a.td_abs[d.b] = fabsf(r - q_sa);
    a.loss[d.b] = d.w * ce;
  }
  return d.valid ? d.w * (p_sa - m) * a.grad_scale : 0.f;
}

template <bool RESCALE>
__global__ void __launch_bounds__(DIST_NT) c51_head_kernel(C51Args ka) {
  extern __shared__ __attribute__((aligned(16))) float c51_smem[];
  const HeadIO& a = ka.io;
  const int N = ka.N;
  dist_head_frame(a, N, c51_smem, [&](const DistSample& d, const float* Ls, int Jp, int lane) {
    constexpr int SPB = DIST_SPB;
    const float delta = (ka.vmax - ka.vmin) / (float)(N - 1);
    const float z = ka.vmin + (float)lane * delta;
    const int astar = c51_astar(Ls + (SPB + d.s) * Jp, a.Pon, a.A, N, lane, z);
    // the target net's distribution of a*, projected onto the support
    const DistRow rg = dist_row(Ls + (2 * SPB + d.s) * Jp, a.Ptg, a.A, N, lane);
    float p, lp, m = 0.f;
    c51_action(rg, astar, N, lane, z, p, lp);
    const float pj = d.valid ? p : 0.f;
    float tz0;
    if constexpr (RESCALE) tz0 = value_rescale_target(d.rew, d.gam, z, a.rescale_eps);
    else tz0 = d.rew + d.gam * z;
    const float tz = fminf(fmaxf(tz0, ka.vmin), ka.vmax);
    const float bj = (tz - ka.vmin) / delta;
    const float fi = (float)lane;
    for (int j = 0; j < N; ++j) {      // increasing j: the oracle's order
      const float pp = __shfl(pj, j, 64), bb = __shfl(bj, j, 64);
      m += pp * fmaxf(0.f, 1.f - fabsf(bb - fi));
    }
    if (!d.valid) m = 0.f;
    return c51_st_pass(a, d, Ls + d.s * Jp, N, lane, z, m, [&] { return wave_sum_dpp(m * z); });
  });
}

APEX_EXPORT int apex_c51_head(C51Args a, hipStream_t st) {
  size_t lds = 0;
  if (!dist_head_args_ok(a.io, a.N, &lds) || !(a.vmin < a.vmax)) return (int)hipErrorInvalidValue;
  return dist_head_launch(c51_head_kernel<true>, c51_head_kernel<false>, a, lds, st);
}

// Histogram-loss (HL-Gauss) target on the same head (Runtime.dist_head = "hl_gauss"; Imani & White 2018,
// Farebrother et al. 2024): the softmax, the support, q, a* and the gradient are the categorical head's; the
// target row is the scalar double-DQN target spread over the bins as a Gaussian (no projection):
//
//   sigma = sigma_ratio delta,   e_i = v_min + (i - 1/2) delta, i = 0..N   (bin i = [e_i, e_i+1], centre z_i)
//   y     = clamp(R + G q_target(S_t+n)[a*], v_min, v_max)      (RESCALE: T(R, G, q_target[a*]), value_rescale.h)
//   E_i   = erf((e_i - y) / (sigma sqrt 2)),   m_i = (E_i+1 - E_i) / (E_N - E_0)
//   loss_b = -w_b sum_i m_i log p(S_t)[a_b,i],  td_abs_b = |y - q(S_t)[a_b]|,  g_i = w_b (p - m_i) grad_scale
//
// e_i, sigma, E_i and the quotient are fp64 on the fp32 v_min, v_max, sigma_ratio and y; m_i is rounded to fp32
// once (value_rescale.h's convention).  y is clamped, so E_N - E_0 is at least the mass of half a bin.  A lane
// evaluates its bin's two edges: (i + 1) - 1/2 and i + 1/2 are the same fp64 number, so the masses telescope.
struct HlgArgs {
  HeadIO io;            // as C51Args
  int N;
  float vmin, vmax, sigma_ratio;
};
static_assert(std::is_standard_layout_v<HlgArgs> && std::is_trivially_copyable_v<HlgArgs>);

template <bool RESCALE>
__global__ void __launch_bounds__(DIST_NT) hlg_head_kernel(HlgArgs ka) {
  extern __shared__ __attribute__((aligned(16))) float c51_smem[];
  const HeadIO& a = ka.io;
  const int N = ka.N;
  dist_head_frame(a, N, c51_smem, [&](const DistSample& d, const float* Ls, int Jp, int lane) {
    constexpr int SPB = DIST_SPB;
    const float delta = (ka.vmax - ka.vmin) / (float)(N - 1);
    const float z = ka.vmin + (float)lane * delta;
    const int astar = c51_astar(Ls + (SPB + d.s) * Jp, a.Pon, a.A, N, lane, z);
    // the scalar target from the target net's expectation of a*, then its Gaussian mass per bin
    const DistRow rg = dist_row(Ls + (2 * SPB + d.s) * Jp, a.Ptg, a.A, N, lane);
    float p, lp;
    const float qg = c51_action(rg, astar, N, lane, z, p, lp);
    float y0;
    if constexpr (RESCALE) y0 = value_rescale_target(d.rew, d.gam, qg, a.rescale_eps);
    else y0 = d.rew + d.gam * qg;
    const float y = fminf(fmaxf(y0, ka.vmin), ka.vmax);
    const double vmin = (double)ka.vmin;
    const double dl = ((double)ka.vmax - vmin) / (double)(N - 1);
    const double inv = 1.0 / ((double)ka.sigma_ratio * dl * 1.4142135623730951);
    const double i0 = (double)min(lane, N - 1);            // (a lane past N repeats the last bin)
    const double Elo = erf((vmin + (i0 - 0.5) * dl - (double)y) * inv);
    const double Ehi = erf((vmin + (i0 + 0.5) * dl - (double)y) * inv);
    const double E0 = __shfl(Elo, 0, 64), EN = __shfl(Ehi, N - 1, 64);
    const float m = d.valid ? (float)((Ehi - Elo) / (EN - E0)) : 0.f;
    return c51_st_pass(a, d, Ls + d.s * Jp, N, lane, z, m, [&] { return y; });
  });
}

APEX_EXPORT int apex_hlg_head(HlgArgs a, hipStream_t st) {
  size_t lds = 0;
  if (!dist_head_args_ok(a.io, a.N, &lds) || !(a.vmin < a.vmax) || !(a.sigma_ratio > 0.f) || !std::isfinite(a.sigma_ratio))
    return (int)hipErrorInvalidValue;
  return dist_head_launch(hlg_head_kernel<true>, hlg_head_kernel<false>, a, lds, st);
}

// Actor side: expected q of the distributional head + epsilon-greedy, one wave per env row
// (four per block; a wave past E repeats the last row and stores nothing).
__global__ void __launch_bounds__(256) c51_actor_head_kernel(C51ActorArgs ka) {
  const ActorIO& a = ka.io;
  extern __shared__ __attribute__((aligned(16))) float c51_smem[];
  const int lane = threadIdx.x & 63;
  const int A = a.A, N = ka.N;
  int e; bool live;
  const float* L = dist_actor_open(a, N, c51_smem, lane, threadIdx.x >> 6, e, live);
  const float delta = (ka.vmax - ka.vmin) / (float)(N - 1);
  const float z = ka.vmin + (float)lane * delta;
  const DistRow r = dist_row(L, a.P, A, N, lane);
  int best = 0;
  float bq = -3.4e38f, p, lp;
  for (int j = 0; j < A; ++j) {
    const float q = c51_action(r, j, N, lane, z, p, lp);
    if (q > bq) { bq = q; best = j; }
    if (live && lane == 0) a.q_out[(int64_t)e * A + j] = q;
  }
  if (live && lane == 0) dist_actor_draw(best, e, A, a.eps, a.seed, a.ctr, a.a_out);
}

APEX_EXPORT int apex_c51_actor_head(C51ActorArgs a, hipStream_t st) {
  size_t lds = 0;
  if (!dist_actor_args_ok(a.io, a.N, &lds) || !(a.vmin < a.vmax)) return (int)hipErrorInvalidValue;
  c51_actor_head_kernel<<<(a.io.E + 3) / 4, 256, lds, st>>>(a);
  APEX_CHECK_LAUNCH();
}
