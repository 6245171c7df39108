// Fused dueling heads + n-step double-DQN target + Huber/IS loss + priorities
// + head backward.  One block of three waves per sample: each wave evaluates
// one 2*HS-wide activation row (online S_t, online S_t+n, target S_t+n; HS =
// stream width, 512 for the NatureCNN, 256 for IMPALA) and
// the q-values meet in LDS; wave 0 finishes loss, priority and backward.
//
// Covers reference duelling_network.py:18-19,25-27 (value/advantage heads and
// the dueling combine, with the per-sample advantage mean instead of the
// batch-global sum, defect A15) and learner.py:43-50 (DDQN target from the
// online argmax and the target net's value, TD error, loss, priorities) plus
// the loss gradient back to the 1024-wide stream activations -- work that the
// reference spreads over ~20 separate torch ops.
//
// Inputs (per sample b of the local batch B):
//   Hon  [2B,1024] bf16  online stream activations (post-ReLU): rows [0,B) = S_t,
//                        rows [B,2B) = S_{t+n}; cols [0,512) value, [512,1024) adv
//   Htg  [B,1024]  bf16  target-network stream activations for S_{t+n}
//   head params fp32: wv[512] bv[1] wa[A,512] ba[A] (online, target)
//   act int32, rew/gam/isw fp32
// Outputs: td_abs[B], loss[B], q_t[B,A] (optional), dH[B,1024] bf16 (gradient
// at the pre-ReLU stream outputs), dhead[B,1+A] fp32 (d value, d advantage).
#include "ddqn_args.h"

// hp.part != null: the fc forward's split-K epilogue runs inside (head_common.h
// load_row_part); blocks >= B run the conv2 weight-fragment pack job (pk.out != null)
// that otherwise rides on that epilogue's launch.
// RESCALE: the rescaled target (csrc/value_rescale.h, eps = io.rescale_eps); everything else is the plain code.
template <int HS, int MAXA, bool RESCALE>
__global__ void __launch_bounds__(192) ddqn_head_kernel(DdqnArgs ka) {
  const HeadIO& a = ka.io;
  const int B = a.B;
  if ((int)blockIdx.x >= B) {
    for (int i = ((int)blockIdx.x - B) * 192 + (int)threadIdx.x; i < C2D_PACK_THREADS; i += ((int)gridDim.x - B) * 192)
      pack_c2d_wfrag_word(i, ka.pk.w, ka.pk.w_lo, ka.pk.out);
    return;
  }
  float ad;
  const bool w0 = ddqn_head_body<HS, MAXA, false, RESCALE>(a, ka.huber, ka.kappa, &ad, ka.hp);
  // batch-max IS normalisation: block 0's second wave
  if (!w0 && (a.isn.out != nullptr || a.isn.valid_count != nullptr) && blockIdx.x == 0 && (threadIdx.x >> 6) == 1)
    head_is_norm(a, threadIdx.x & 63);
}

// (h.NV >= 2: the wide head of csrc/c51_head.hip, blockIdx.x = row tile)
__global__ void __launch_bounds__(512) head_wgrad_kernel(HeadWgArgs h) {
  if (h.NV >= 2) head_wgrad_wide_body(h, blockIdx.x, blockIdx.y, blockIdx.x * gridDim.y + blockIdx.y);
  else head_wgrad_body(h, blockIdx.x, blockIdx.y);
}

APEX_EXPORT int apex_ddqn_head(DdqnArgs a, hipStream_t st) {
  const HeadIO& io = a.io;
  if (!head_io_ok(io) || (io.zero_ptr != nullptr && io.zero_n < 0)) return (int)hipErrorInvalidValue;
  // 16-byte row loads / stores of the 512-wide streams (head_io_ok asks for 8)
  if (io.hidden == 512 && (((uintptr_t)io.Hon | (uintptr_t)io.Htg | (uintptr_t)io.dH | (uintptr_t)io.lo.Hon |
                            (uintptr_t)io.lo.Htg | (uintptr_t)io.lo.dH) & 15))
    return (int)hipErrorInvalidValue;
  if (const HeadPart& hp = a.hp; hp.part != nullptr) {   // partials [nz][3B][2 hidden]; rows [0, B) of h go to hp.hon
    if (hp.nz < 1 || hp.hon == nullptr || hp.bias_on == nullptr || hp.bias_tg == nullptr || hp.two_b != 2 * io.B ||
        (io.lo.Hon != nullptr) != (hp.hon_lo != nullptr) || (((uintptr_t)hp.part | (uintptr_t)hp.hon) & 15))
      return (int)hipErrorInvalidValue;
  }
  if (a.pk.out != nullptr && (a.pk.w == nullptr || ((uintptr_t)a.pk.out & 15))) return (int)hipErrorInvalidValue;
  const int grid = io.B + (a.pk.out != nullptr ? 128 : 0);
  const bool rs = io.rescale_eps > 0.f;       // 0 = the plain double-DQN target
#define APEX_HEAD_LAUNCH(HS_, MA_, RS_) ddqn_head_kernel<HS_, MA_, RS_><<<grid, 192, 0, st>>>(a)
  // the q arrays in registers: 8 actions (every ALE minimal action set but the full
  // 18) keep the kernel free of scratch
  // (the rescaled target is the NatureCNN learner's: no 256-wide instantiation, whose MAXA = 32 form would spill)
  if (rs && io.hidden != 512) return (int)hipErrorInvalidValue;
  if (rs && io.A <= 8) APEX_HEAD_LAUNCH(512, 8, true);
  else if (rs) APEX_HEAD_LAUNCH(512, HEAD_MAXA, true);
  else if (io.hidden == 512 && io.A <= 8) APEX_HEAD_LAUNCH(512, 8, false);
  else if (io.hidden == 512) APEX_HEAD_LAUNCH(512, HEAD_MAXA, false);
  else if (io.hidden == 256 && io.A <= 8) APEX_HEAD_LAUNCH(256, 8, false);
  else if (io.hidden == 256) APEX_HEAD_LAUNCH(256, HEAD_MAXA, false);
  else
    return (int)hipErrorInvalidValue;
#undef APEX_HEAD_LAUNCH
  APEX_CHECK_LAUNCH();
}

// Element-wise probe of csrc/value_rescale.h for the unit test: out[i] = T(R[i], Gamma[i], y[i], eps).
__global__ void __launch_bounds__(256) value_rescale_probe_kernel(const float* __restrict__ y, const float* __restrict__ R,
                                                                  const float* __restrict__ G, float eps,
                                                                  float* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = value_rescale_target(R[i], G[i], y[i], eps);
}

APEX_EXPORT int apex_value_rescale_probe(const float* y, const float* R, const float* Gamma, float eps, float* out,
                                         int64_t n, hipStream_t st) {
  if (y == nullptr || R == nullptr || Gamma == nullptr || out == nullptr || n < 1 || n > (int64_t)1 << 30 ||
      !(eps > 0.f && eps <= 1.f))
    return (int)hipErrorInvalidValue;
  value_rescale_probe_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(y, R, Gamma, eps, out, n);
  APEX_CHECK_LAUNCH();
}

// h.NV >= 2: NV value rows and A advantage rows (the distributional head: dhead [B, NV + A])
APEX_EXPORT int apex_head_wgrad(HeadWgArgs h, hipStream_t st) {
  if (!head_wg_args_ok(h)) return (int)hipErrorInvalidValue;
  head_wgrad_kernel<<<dim3(head_wg_rows(h), h.HS / 64), 512, 0, st>>>(h);
  APEX_CHECK_LAUNCH();
}

// Actor-side: dueling q from stream activations + epsilon-greedy selection.
// One wave per env row. eps per row; uniform draws from the counter RNG.
// H_lo (fp32 learner, split mode): the lo plane of the stream activations, so the
// actor's q-values (and the initial priorities built from them) are fp32-accurate.
template <int HS, int MAXA>
__global__ void __launch_bounds__(256) actor_head_kernel(ActorIO a) {
  const int A = a.A;
  const int lane = threadIdx.x & 63;
  const int e = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (e >= a.E) return;
  float q[MAXA], hv[HS / 64], ha[HS / 64];
  head_row<HS, MAXA>(a.H + (int64_t)e * 2 * HS, a.H_lo != nullptr ? a.H_lo + (int64_t)e * 2 * HS : nullptr, a.P, A, lane,
                     q, hv, ha);
  int best = 0;
  float bq = -3.4e38f;
#pragma unroll
  for (int j = 0; j < MAXA; ++j)
    if (j < A && q[j] > bq) { bq = q[j]; best = j; }
  if (lane < A) {
    float qv = 0.f;
#pragma unroll
    for (int j = 0; j < MAXA; ++j)
      if (j == lane) qv = q[j];
    a.q_out[(int64_t)e * A + lane] = qv;
  }
  if (lane == 0) dist_actor_draw(best, e, A, a.eps, a.seed, a.ctr, a.a_out);
}

APEX_EXPORT int apex_actor_head(ActorIO a, hipStream_t st) {
  if (!actor_io_ok(a)) return (int)hipErrorInvalidValue;
  // 16-byte row loads of the 512-wide streams (actor_io_ok asks for 8)
  if (a.hidden == 512 && (((uintptr_t)a.H | (uintptr_t)a.H_lo) & 15)) return (int)hipErrorInvalidValue;
#define APEX_ACTOR_HEAD(HS_, MA_) actor_head_kernel<HS_, MA_><<<(a.E + 3) / 4, 256, 0, st>>>(a)
  if (a.hidden == 512 && a.A <= 8) APEX_ACTOR_HEAD(512, 8);
  else if (a.hidden == 512) APEX_ACTOR_HEAD(512, HEAD_MAXA);
  else if (a.hidden == 256 && a.A <= 8) APEX_ACTOR_HEAD(256, 8);
  else if (a.hidden == 256) APEX_ACTOR_HEAD(256, HEAD_MAXA);
  else return (int)hipErrorInvalidValue;
#undef APEX_ACTOR_HEAD
  APEX_CHECK_LAUNCH();
}
