// Wide quantile-regression (QR-DQN) head: Runtime.dist_head = "quantile" with 65 <= N <= 256 quantiles per
// action (the paper's N = 200), and any 2 <= N <= 256 under the `qr_wide` switch.  The definitions are
// csrc/qr_head.hip's (theta, q, a*, T_j, the quantile Huber loss with its j-sums in increasing j, dhead, td_abs,
// dH); the head weights are read as there: wv [N][512], bv [N], wa [A N][512], ba [A N], fp32.
//
// qr_head_kernel maps one lane to one quantile and forms the (A + 1) N logits as fp32 VALU dot products in the
// LDS of a two-sample block; neither survives N > 64.  Here the head is three launches on one stream:
//
//   qr_wide_logits_kernel   csrc/wide_head.h: L [3B][Jp] = H . W^T without biases, an MFMA GEMM into the fp32 workspace
//   qr_wide_finish_kernel   <RESCALE, NQ> one wave per sample, four per block.  Lane l owns quantiles l, l + 64,
//                           .. (NQ = ceil(N / 64) register sets; a quantile past N holds theta = T = 0 and is
//                           masked out of every sum).  theta, q (lane partial over its sets, then a wave sum), a*
//                           (first maximum), T; the j loop runs in increasing j and reads T_j with a wave-uniform
//                           readlane from register set j / 64 while each lane accumulates rho and the clamp term
//                           of its NQ quantiles.  Writes td_abs, loss, q_out and the dhead row [(A + 1) N].  It
//                           carries dist_head_side's duties: the head-gradient region is zeroed by all blocks,
//                           the IsNorm statistic is left by block 0's last wave.
//   qr_wide_dh_kernel       csrc/wide_head.h: dH [B][1024] = relu'(h) (dhead . W) per stream as an MFMA GEMM
//
// The actor side is the logits kernel with one weight set on the E env rows and qr_wide_actor_finish_kernel: one
// wave per row, q = the mean of theta, then dist_actor_draw with qr_actor_head_kernel's counter-RNG words.
// Nothing depends on the order blocks run in (no float atomics).
#include "wide_head.h"

struct QRWideArgs {
  HeadIO io;            // as QRArgs.io
  int N;
  float kappa;
  float* L;             // [3B][Jp] fp32 logits workspace (qr_wide_jp)
};
struct QRWideActorArgs {
  ActorIO io;
  int N;
  float* L;             // [E][Jp]
};
static_assert(std::is_standard_layout_v<QRWideArgs> && std::is_trivially_copyable_v<QRWideArgs> &&
              std::is_standard_layout_v<QRWideActorArgs> && std::is_trivially_copyable_v<QRWideActorArgs>);

// q of action j: this lane's partial over its sets, then the wave sum
template <int NQ>
__device__ __forceinline__ float qw_q(const QWRow<NQ>& r, int j, int N, int lane, float invN, float* th) {
  float p = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    th[s] = qw_theta(r, j, s, N, lane);
    p += th[s];
  }
  return wave_sum_dpp(p) * invN;
}

template <bool RESCALE, int NQ>
__global__ void __launch_bounds__(QW_NT) qr_wide_finish_kernel(QRWideArgs ka) {
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
  const float invN = 1.0f / (float)N, kappa = ka.kappa;
  float th[NQ];
  // double DQN: a* from the online net at S_t+n (first maximum wins)
  int astar = 0;
  {
    const QWRow<NQ> rn = qw_row<NQ>(ka.L + (int64_t)(B + b) * Jp, a.Pon, A, N, lane);
    float best = -3.4e38f;
    for (int j = 0; j < A; ++j) {
      const float q = qw_q(rn, j, N, lane, invN, th);
      if (q > best) { best = q; astar = j; }
    }
    astar = __builtin_amdgcn_readfirstlane(astar);
  }
  // the target samples: register set s of lane l holds T_(64 s + l)
  float T[NQ];
  {
    const QWRow<NQ> rg = qw_row<NQ>(ka.L + (int64_t)(2 * B + b) * Jp, a.Ptg, A, N, lane);
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const float tg = qw_theta(rg, astar, s, N, lane);
      const bool ok = 64 * s + lane < N;
      if constexpr (RESCALE) T[s] = ok ? value_rescale_target(rew, gam, tg, a.rescale_eps) : 0.f;
      else T[s] = ok ? rew + gam * tg : 0.f;
    }
  }
  // S_t: q of every action, the taken action's quantiles
  float th_sa[NQ], q_sa = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) th_sa[s] = 0.f;
  {
    const QWRow<NQ> rt = qw_row<NQ>(ka.L + (int64_t)b * Jp, a.Pon, A, N, lane);
    for (int j = 0; j < A; ++j) {
      const float q = qw_q(rt, j, N, lane, invN, th);
      if (a.q_out != nullptr && live && lane == 0) a.q_out[(int64_t)b * A + j] = q;
      if (j == a_b) {
        q_sa = q;
#pragma unroll
        for (int s = 0; s < NQ; ++s) th_sa[s] = th[s];
      }
    }
  }
  // this lane's quantiles against every target sample, in increasing j
  float tau[NQ], rho[NQ], c[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    tau[s] = (2.f * (float)(64 * s + lane) + 1.f) / (2.f * (float)N);
    rho[s] = c[s] = 0.f;
  }
  float tsum = 0.f;                      // RESCALE: sum_j T_j in increasing j (the oracle's order)
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
  float rs = 0.f, ts = 0.f;
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    rs += 64 * s + lane < N ? rho[s] * sc : 0.f;
    ts += T[s];
  }
  const float ls = wave_sum_dpp(rs);
  float et;
  if constexpr (RESCALE) et = tsum * invN;
  else et = wave_sum_dpp(ts) * invN;
  if (live && lane == 0) {
    a.td_abs[b] = fabsf(et - q_sa);
    a.loss[b] = w * ls;
  }
  // the dhead row: d v[i] = g_i, d adv[j, i] = g_i ([j = a_b] - 1 / A)
  if (live) {
    float* __restrict__ dh = a.dhead + (int64_t)b * J;
    const float invA = 1.0f / (float)A;
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const int i = 64 * s + lane;
      if (i >= N) continue;
      const float g = -w * a.grad_scale * (c[s] * sc);
      dh[i] = g;
      for (int j = 0; j < A; ++j) dh[N + j * N + i] = g * ((j == a_b ? 1.f : 0.f) - invA);
    }
  }
  // batch-max IS statistic: block 0's last wave
  if ((a.isn.out != nullptr || a.isn.valid_count != nullptr) && blockIdx.x == 0 && wv == QW_NT / 64 - 1)
    head_is_norm(a, lane);
}

// ------------------------------------------------------------------------------------------------ actor
// q = mean of the quantiles + epsilon-greedy, one wave per env row (four per block; a wave past E repeats the last
// row and stores nothing); NQ = ceil(N / 64) register sets, as in the learner's finish kernel
template <int NQ>
__global__ void __launch_bounds__(QW_NT) qr_wide_actor_finish_kernel(QRWideActorArgs ka) {
  const ActorIO& a = ka.io;
  const int lane = threadIdx.x & 63;
  const int A = a.A, N = ka.N;
  const int e_raw = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = e_raw < a.E;
  const int e = min(e_raw, a.E - 1);
  const float invN = 1.0f / (float)N;
  const QWRow<NQ> r = qw_row<NQ>(ka.L + (int64_t)e * qr_wide_jp(A, N), a.P, A, N, lane);
  int best = 0;
  float bq = -3.4e38f, th[NQ];
  for (int j = 0; j < A; ++j) {
    const float q = qw_q(r, j, N, lane, invN, th);
    if (q > bq) { bq = q; best = j; }
    if (live && lane == 0) a.q_out[(int64_t)e * A + j] = q;
  }
  if (live && lane == 0) dist_actor_draw(best, e, A, a.eps, a.seed, a.ctr, a.a_out);
}

// ------------------------------------------------------------------------------------------------ launchers
template <bool RESCALE>
static inline void qw_finish_launch(const QRWideArgs& a, hipStream_t st) {
  const int grid = (a.io.B + 3) / 4;
  switch ((a.N + 63) / 64) {
    case 1: qr_wide_finish_kernel<RESCALE, 1><<<grid, QW_NT, 0, st>>>(a); break;
    case 2: qr_wide_finish_kernel<RESCALE, 2><<<grid, QW_NT, 0, st>>>(a); break;
    case 3: qr_wide_finish_kernel<RESCALE, 3><<<grid, QW_NT, 0, st>>>(a); break;
    default: qr_wide_finish_kernel<RESCALE, 4><<<grid, QW_NT, 0, st>>>(a); break;
  }
}

APEX_EXPORT int apex_qr_wide_head(QRWideArgs a, hipStream_t st) {
  if (!qw_head_ok(a.io, a.N, a.L) || !(a.kappa > 0.f)) return (int)hipErrorInvalidValue;
  qw_launch_head_logits(a.io, a.N, a.L, st);
  if (a.io.rescale_eps > 0.f) qw_finish_launch<true>(a, st);
  else qw_finish_launch<false>(a, st);
  qw_launch_dh(a.io, a.N, st);
  APEX_CHECK_LAUNCH();
}

static inline void qw_actor_finish_launch(const QRWideActorArgs& a, hipStream_t st) {
  const int grid = (a.io.E + 3) / 4;
  switch ((a.N + 63) / 64) {
    case 1: qr_wide_actor_finish_kernel<1><<<grid, QW_NT, 0, st>>>(a); break;
    case 2: qr_wide_actor_finish_kernel<2><<<grid, QW_NT, 0, st>>>(a); break;
    case 3: qr_wide_actor_finish_kernel<3><<<grid, QW_NT, 0, st>>>(a); break;
    default: qr_wide_actor_finish_kernel<4><<<grid, QW_NT, 0, st>>>(a); break;
  }
}

APEX_EXPORT int apex_qr_wide_actor_head(QRWideActorArgs a, hipStream_t st) {
  const ActorIO& io = a.io;
  if (!qw_actor_ok(io, a.N, a.L)) return (int)hipErrorInvalidValue;
  qw_launch_actor_logits(io, a.N, a.L, st);
  qw_actor_finish_launch(a, st);
  APEX_CHECK_LAUNCH();
}

// The finish alone, on logits the caller has written into L (csrc/noisy_actor.hip noisy_env_logits_kernel: the
// per-env noisy logits; io.P then carries the mu biases, io.H is not read)
APEX_EXPORT int apex_qr_wide_actor_finish(QRWideActorArgs a, hipStream_t st) {
  if (!qw_actor_ok(a.io, a.N, a.L)) return (int)hipErrorInvalidValue;
  qw_actor_finish_launch(a, st);
  APEX_CHECK_LAUNCH();
}

// floats per row of the logits workspace; sizeof the two argument blocks (which = 0 / 1) for the ctypes mirrors
APEX_EXPORT int apex_qr_wide_jp(int A, int N) { return qr_wide_jp(A, N); }
APEX_EXPORT int apex_qr_wide_args_size(int which) {
  return which == 0 ? (int)sizeof(QRWideArgs) : (int)sizeof(QRWideActorArgs);
}
