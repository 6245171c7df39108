// Fused dueling heads + Munchausen-DQN target (Vieillard, Pietquin, Geist 2020) + Huber/IS loss +
// priorities + head backward: the scalar head of csrc/ddqn_head.hip with another target.  One block
// of three waves per sample, each wave evaluating one 2*HS-wide activation row:
//   wave 0  online net at S_t      (q_on, keeps the weights the backward needs)
//   wave 1  target net at S_t+n    (g1)
//   wave 2  target net at S_t      (g0)
// The q-vectors meet in LDS; wave 0 forms, with pi = softmax(g / tau) and every exponent max-subtracted
// (no overflow; a term that underflows to 0 is the correct limit),
//   tau ln pi(a | g0) = (g0[a] - max g0) - tau ln sum_a' exp((g0[a'] - max g0) / tau)
//   bonus = alpha clamp(tau ln pi(a | g0), clip, 0)
//   vsoft = max g1 + tau ln sum_a' exp((g1[a'] - max g1) / tau)     (= E_pi[g1 - tau ln pi(. | g1)])
//   T     = rew + bonus + gam vsoft,   delta = T - q_on[a]
// and runs the scalar head's own loss / dhead / dH tail (head_common.h ddqn_head_body<.., MDQN = true>).  There is no
// online argmax: the target is detached, the gradient flows through q_on[a] only.  learner/losses.py
// munchausen_loss is the definition, TorchBackend.mdqn_head the oracle.
//
// Inputs (per sample b of the batch B):
//   Hon  [B, 2 HS]   bf16  online stream activations of S_t; cols [0, HS) value, [HS, 2 HS) advantage
//   Htg  [2B, 2 HS]  bf16  target stream activations: rows [0, B) = S_t+n, rows [B, 2B) = S_t
//   lo.Hon / lo.Htg / lo.dH: the lo planes in split (fp32-accurate) mode, else null
// Outputs: td_abs[B], loss[B], q_out[B, A] (optional), aux[B, 2] = (bonus, vsoft) (optional),
// dH[B, 2 HS], dhead[B, 1 + A]; the side duties of ddqn_head_kernel (head-gradient zeroing, IsNorm).
#include "head_common.h"

struct MdqnArgs {
  HeadIO io;             // Hon [B], Htg [2B]; dhead [B][1 + A]
  int huber;
  float kappa, alpha, tau, clip;
  float* aux;            // [B, 2] (bonus, vsoft), or null
  HeadPart hp;           // must be all null: the deferred fc epilogue is not taken (see mdqn_head_kernel)
};
static_assert(std::is_standard_layout_v<MdqnArgs> && std::is_trivially_copyable_v<MdqnArgs>);

// ddqn_head_body<HS, MAXA, true> (head_common.h) with the side job of ddqn_head_kernel's second wave.  The body
// is instantiated with its HeadPart argument taken from the launch arguments, as ddqn_head_kernel does, although
// the launcher only lets a null one through: with both of the body's forward paths present hipcc compiles wave
// 0's head_q as it does in ddqn_head_kernel, and q_out is bit-equal to that kernel's (with the path folded away
// two products of the value stream's dot product contract differently, one unit in the last place of q).
template <int HS, int MAXA>
__global__ void __launch_bounds__(192) mdqn_head_kernel(MdqnArgs ka) {
  const HeadIO& a = ka.io;
  float ad;
  const MdqnTarget mt{ka.alpha, ka.tau, ka.clip, ka.aux};
  const bool w0 = ddqn_head_body<HS, MAXA, true>(a, ka.huber, ka.kappa, &ad, ka.hp, &mt);
  // batch-max IS normalisation: block 0's second wave (csrc/ddqn_head.hip, same semantics)
  if (!w0 && (a.isn.out != nullptr || a.isn.valid_count != nullptr) && blockIdx.x == 0 && (threadIdx.x >> 6) == 1)
    head_is_norm(a, threadIdx.x & 63);
}

APEX_EXPORT int apex_mdqn_head(MdqnArgs a, hipStream_t st) {
  const HeadIO& io = a.io;
  if (!head_io_ok(io) || io.hidden != 512) return (int)hipErrorInvalidValue;
  if (!(a.tau > 0.f) || !(a.clip < 0.f) || !(a.alpha >= 0.f && a.alpha <= 1.f)) return (int)hipErrorInvalidValue;
  if (io.zero_ptr != nullptr && io.zero_n < 0) return (int)hipErrorInvalidValue;
  if (a.hp.part != nullptr || a.hp.hon != nullptr || a.hp.hon_lo != nullptr) return (int)hipErrorInvalidValue;
  if (io.rescale_eps != 0.f) return (int)hipErrorInvalidValue;      // the Munchausen target is not rescaled
  // 16-byte row loads / stores (head_io_ok asks for 8)
  if (((uintptr_t)io.Hon | (uintptr_t)io.Htg | (uintptr_t)io.dH | (uintptr_t)io.lo.Hon | (uintptr_t)io.lo.Htg |
       (uintptr_t)io.lo.dH) & 15)
    return (int)hipErrorInvalidValue;
  // the q arrays in registers: 8 actions keep the kernel free of scratch (as ddqn_head_kernel)
  if (io.A <= 8) mdqn_head_kernel<512, 8><<<io.B, 192, 0, st>>>(a);
  else mdqn_head_kernel<512, HEAD_MAXA><<<io.B, 192, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}
