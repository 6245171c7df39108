// Quantile-regression (QR-DQN) dueling head for the NatureCNN learner: the distributional
// head of Runtime.dist_head = "quantile" (Runtime.num_atoms = N quantiles per action, one
// lane per quantile, 2 <= N <= 64).  No support: nothing to clamp onto.
//
// Head weights exactly as csrc/c51_head.hip reads them: wv [N][HS], bv [N], wa [A N][HS]
// (row a N + i = action a, quantile i), ba [A N]; HS = 512.  kappa = Runtime.huber_delta > 0.
//
//   theta[a,i] = v[i] + adv[a,i] - mean_a' adv[a',i]         (dueling mean per quantile)
//   q[a]       = (1/N) sum_i theta[a,i],   tau_i = (2 i + 1) / (2 N)
//   a*         = argmax_a q_online(S_t+n) (first maximum)
//   T_j        = R + G theta_target(S_t+n)[a*,j]             (G = 0 at terminals: T_j = R)
//   u_ij       = T_j - theta(S_t)[a_b,i]
//   L(u)       = u^2 / 2 if |u| <= kappa, else kappa (|u| - kappa / 2)
//   loss_b     = w_b sum_i (1/N) sum_j |tau_i - 1{u_ij < 0}| L(u_ij) / kappa
//   g_i        = -w_b grad_scale (1/N) sum_j |tau_i - 1{u_ij < 0}| clamp(u_ij, -kappa, kappa) / kappa
//                (the j-sums in increasing j; the i-sum a wave sum)
//   d v[i] = g_i,  d adv[a,i] = g_i ([a = a_b] - 1/A)  -> dhead [B][(A + 1) N]
//   td_abs_b   = |(1/N) sum_j T_j - q(S_t)[a_b]| = |R + G q_target[a*] - q[a_b]|
// Runtime.value_rescale (qr_head_kernel<true>, HeadIO.rescale_eps > 0): T_j = h(R + G h^-1(theta_target[a*,j])) per
// target sample (csrc/value_rescale.h; exact for quantiles, h being increasing) and td_abs_b takes the mean of the
// transformed T_j, summed in increasing j -- the shortcut through q_target no longer equals it.
//   dH         = dhead . W, masked by the stream ReLUs (bf16, or hi / lo planes)
//
// qr_head_kernel: one block of DIST_NT threads per DIST_SPB samples, run by csrc/dist_head.h's
// dist_head_frame (staging the activation rows, the logits, the sample's batch row, the dhead
// row and dH: shared with the categorical heads).  The kernel hands the frame its phase 2:
//   2. Wave s finishes sample s with lane = quantile.  The three theta rows come from the
//      LDS logits; q per action is one wave sum; a* is made wave-uniform; each lane keeps
//      its T_j, and the j loop reads lane j of it (j is wave-uniform: a lane read, no
//      shuffle) while every lane accumulates its own quantile's loss and gradient.  Lanes
//      >= N hold theta = T = 0 and add exact zeros to the wave sums; a sample past the
//      batch stores nothing.
// Nothing depends on the order blocks run in (no float atomics).
//
// qr_actor_head_kernel: one wave per env row, the logits as in phase 1 with the row in
// registers, q = the mean of theta per action and the epsilon-greedy draw of
// actor_head_kernel (same counter-RNG words).
#include "dist_head.h"

struct QRArgs {
  HeadIO io;            // Hon [2B], Htg [B]; q_out the q(S_t) = mean of the quantiles; dhead [B][(A + 1) N]
  int N;
  float kappa;
};
static_assert(std::is_standard_layout_v<QRArgs> && std::is_trivially_copyable_v<QRArgs>);

// this lane's quantile of action a (0 in a lane past N)
__device__ __forceinline__ float qr_theta(const DistRow& r, int a, int N, int lane) {
  return lane < N ? r.v + (r.L[N + a * N + lane] + r.ba[a * N + lane]) - r.mean : 0.f;
}

template <bool RESCALE>
__global__ void __launch_bounds__(DIST_NT) qr_head_kernel(QRArgs ka) {
  extern __shared__ __attribute__((aligned(16))) float qr_smem[];
  const HeadIO& a = ka.io;
  const int N = ka.N;
  dist_head_frame(a, N, qr_smem, [&](const DistSample& d, const float* Ls, int Jp, int lane) {
    constexpr int SPB = DIST_SPB;
    const int A = a.A;
    const float invN = 1.0f / (float)N;
    const float kappa = ka.kappa;
    // double DQN: a* from the online net at S_t+n (first maximum wins)
    int astar = 0;
    {
      const DistRow rn = dist_row(Ls + (SPB + d.s) * Jp, a.Pon, A, N, lane);
      float best = -3.4e38f;
      for (int j = 0; j < A; ++j) {
        const float q = wave_sum_dpp(qr_theta(rn, j, N, lane)) * invN;
        if (q > best) { best = q; astar = j; }
      }
      astar = __builtin_amdgcn_readfirstlane(astar);
    }
    // the target samples: lane j holds T_j
    float T;
    {
      const DistRow rg = dist_row(Ls + (2 * SPB + d.s) * Jp, a.Ptg, A, N, lane);
      if constexpr (RESCALE)
        T = d.valid ? value_rescale_target(d.rew, d.gam, qr_theta(rg, astar, N, lane), a.rescale_eps) : 0.f;
      else
        T = d.valid ? d.rew + d.gam * qr_theta(rg, astar, N, lane) : 0.f;
    }
    // S_t: q of every action, the taken action's quantiles
    float th_sa = 0.f, q_sa = 0.f;
    {
      const DistRow rt = dist_row(Ls + d.s * Jp, a.Pon, A, N, lane);
      for (int j = 0; j < A; ++j) {
        const float th = qr_theta(rt, j, N, lane);
        const float q = wave_sum_dpp(th) * invN;
        if (a.q_out != nullptr && d.live && lane == 0) a.q_out[(int64_t)d.b * A + j] = q;
        if (j == d.a_b) { th_sa = th; q_sa = q; }
      }
    }
    // this lane's quantile against every target sample, in increasing j
    const float tau = (2.f * (float)lane + 1.f) / (2.f * (float)N);
    float rho = 0.f, c = 0.f;
    float tsum = 0.f;                    // RESCALE: sum_j T_j in increasing j (the oracle's order)
    for (int j = 0; j < N; ++j) {
      const float Tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T), j));
      if constexpr (RESCALE) tsum += Tj;
      const float u = Tj - th_sa;
      const float au = fabsf(u);
      const float wgt = fabsf(tau - (u < 0.f ? 1.f : 0.f));
      rho += wgt * (au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa));
      c += wgt * fminf(fmaxf(u, -kappa), kappa);
    }
    const float sc = invN / kappa;
    const float ls = wave_sum_dpp(d.valid ? rho * sc : 0.f);
    float et;
    if constexpr (RESCALE) et = tsum * invN;
    else et = wave_sum_dpp(T) * invN;
    if (d.live && lane == 0) {
      a.td_abs[d.b] = fabsf(et - q_sa);
      a.loss[d.b] = d.w * ls;
    }
    return d.valid ? -d.w * a.grad_scale * (c * sc) : 0.f;
  });
}

APEX_EXPORT int apex_qr_head(QRArgs a, hipStream_t st) {
  size_t lds = 0;
  if (!dist_head_args_ok(a.io, a.N, &lds) || !(a.kappa > 0.f)) return (int)hipErrorInvalidValue;
  return dist_head_launch(qr_head_kernel<true>, qr_head_kernel<false>, a, lds, st);
}

// Actor side: q = mean of the quantiles + epsilon-greedy, one wave per env row (four per
// block; a wave past E repeats the last row and stores nothing).
__global__ void __launch_bounds__(256) qr_actor_head_kernel(QRActorArgs ka) {
  const ActorIO& a = ka.io;
  extern __shared__ __attribute__((aligned(16))) float qr_smem[];
  const int lane = threadIdx.x & 63;
  const int A = a.A, N = ka.N;
  int e; bool live;
  const float* L = dist_actor_open(a, N, qr_smem, lane, threadIdx.x >> 6, e, live);
  const float invN = 1.0f / (float)N;
  const DistRow r = dist_row(L, a.P, A, N, lane);
  int best = 0;
  float bq = -3.4e38f;
  for (int j = 0; j < A; ++j) {
    const float q = wave_sum_dpp(qr_theta(r, j, N, lane)) * invN;
    if (q > bq) { bq = q; best = j; }
    if (live && lane == 0) a.q_out[(int64_t)e * A + j] = q;
  }
  if (live && lane == 0) dist_actor_draw(best, e, A, a.eps, a.seed, a.ctr, a.a_out);
}

APEX_EXPORT int apex_qr_actor_head(QRActorArgs a, hipStream_t st) {
  size_t lds = 0;
  if (!dist_actor_args_ok(a.io, a.N, &lds)) return (int)hipErrorInvalidValue;
  qr_actor_head_kernel<<<(a.io.E + 3) / 4, 256, lds, st>>>(a);
  APEX_CHECK_LAUNCH();
}
