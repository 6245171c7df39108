// Centered RMSprop + global-norm clip + bf16 pack as a block-level device body
// (rmsprop_body), shared by csrc/optimizer.hip (rmsprop_kernel) and by
// csrc/sumtree.hip (rmsprop_sample_kernel: the optimizer launch also draws the
// next step's prioritized batch in its first blocks).
//
// Compile-time variants of the body (OPT_*): the RMSprop update with the learning rate
// frozen at capture (the default: its code is the body of before), the same update
// with a step-indexed learning rate, and Adam.  The last two read the update index
// from device memory (OptSched), so a replayed graph needs no host round trip.
#pragma once
#include <type_traits>
#include "apex_common.h"
#include "cf_pack.h"

#define SQNORM_NPART 1024    // partials apex_grad_sqnorm_partials writes (ops/_lib.py SQNORM_PARTIALS)

// Batch-max IS-weight normalisation (Runtime.is_normalise = "batch_max"): the head
// kernel leaves m = max_j (p_j / p_min)^-beta over the batch (DP: one per rank, in the
// all-gathered shard statistics, stride `wstride`); the loss used the global-min
// weights w_j, so the batch-max weights w_j / m give the gradient g / m -- one scalar
// applied here, before the clip, instead of a second pass over the weights.
__device__ __forceinline__ float is_grad_scale(const double* wnorm, int wn, int wstride) {
  if (wnorm == nullptr) return 1.0f;
  double m = 0.0;
  for (int k = 0; k < wn; ++k) m = fmax(m, wnorm[(int64_t)k * wstride]);
  return m > 0.0 ? (float)(1.0 / m) : 1.0f;
}

// Clip coefficient from the squared-norm partials: every thread of the block sums a
// fixed strided subset, then a fixed-order wave / LDS reduction -- deterministic.
// `gscale` multiplies the gradient first (is_grad_scale); the returned coefficient
// includes it and sh[1] is the norm of the scaled gradient.
// `gpre` (n_pre floats, 16-B aligned, or null): a short gradient range whose squares every
// block sums itself, in the same fixed thread-strided order (the data-parallel step's conv1
// bucket, all-reduced right before this launch: no separate norm launch on the critical
// path, learner/dp_step.py).
__device__ __forceinline__ float clip_coef_from_partials(const double* partials, int npart, float clip,
                                                         float* sh, float gscale = 1.0f,
                                                         const float* gpre = nullptr, int64_t npre = 0) {
  __shared__ double red[16];
  double s = 0.0;
  if (gpre != nullptr) {
    const float4* g4 = reinterpret_cast<const float4*>(gpre);
    const int64_t n4 = npre / 4;
    for (int64_t i = threadIdx.x; i < n4; i += blockDim.x) {
      const float4 v = g4[i];
      s += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
    }
    for (int64_t i = n4 * 4 + threadIdx.x; i < npre; i += blockDim.x) s += (double)gpre[i] * gpre[i];
  }
  for (int i = threadIdx.x; i < npart; i += blockDim.x) s += partials[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    const float norm = (float)sqrt(t) * gscale;
    sh[0] = gscale * ((clip > 0.f) ? fminf(1.0f, clip / (norm + 1e-6f)) : 1.0f);
    sh[1] = norm;
  }
  __syncthreads();
  return sh[0];
}

// ------------------------------------------------------ step-indexed schedules
// The update index inside a replayed graph: the replay's draw counter is bumped once per
// update by the priority write-back (csrc/sumtree.hip ctr_to_bump), in a launch that
// precedes the optimizer launch in stream order; `base` is a device word holding the
// counter's value at update 0 (set at construction / load).  So
//   counter - base     = updates completed, read at the head of an update (a fresh draw),
//   counter - base - 1 = u, the updates completed before the current one, read in its
//                        optimizer launch (whose pre-sample draws update u + 1's batch).
// The optimizer and sample launches only read the counter.
// Both schedules are evaluated in fp64 from the integer index and rounded once to fp32;
// learner/schedules.py is the host mirror (numpy float64, the same operation order: no
// contraction here), bit for bit.
__device__ __forceinline__ float sched_lr(int64_t u, double lr0, double lr_end, int64_t warmup, int64_t decay) {
#pragma clang fp contract(off)
  double lr = lr0;
  if (u < warmup) lr = lr0 * (double)(u + 1) / (double)warmup;
  else if (decay > 0) lr = lr0 + (lr_end - lr0) * fmin(1.0, (double)(u - warmup) / (double)decay);
  return (float)lr;
}

// IS exponent of the batch that update u consumes
__device__ __forceinline__ float sched_beta(int64_t u, double b0, double b_end, int64_t steps) {
#pragma clang fp contract(off)
  const double f = steps > 0 ? fmin(1.0, (double)u / (double)steps) : 1.0;
  return (float)(b0 + (b_end - b0) * f);
}

// b^t in fp64 by squaring (t an integer: at most 2 x 64 multiplications in a fixed
// order, which the host mirror repeats exactly)
__device__ __forceinline__ double pow_u64(double b, uint64_t t) {
#pragma clang fp contract(off)
  double r = 1.0;
  while (t) {
    if (t & 1) r = r * b;
    b = b * b;
    t >>= 1;
  }
  return r;
}

#define OPT_RMSPROP 0        // RMSprop, lr = RmspropArgs.lr
#define OPT_RMSPROP_SCHED 1  // RMSprop, lr(u)
#define OPT_ADAM 2           // Adam, lr(u), bias corrections from t = u + 1 - t0

struct OptSched {
  const uint64_t* ctr;   // the replay's draw counter, or null (OPT_RMSPROP)
  const int64_t* base;   // device word: the counter at update 0
  int adam;              // 1: Adam (RmspropArgs.eps carries adam_eps; alpha / centered unused)
  int64_t warmup, decay; // lr schedule (0: off)
  double lr0, lr_end;
  double beta1, beta2;
  const int64_t* t0;     // device word: the updates completed at the last shrink-and-perturb reset (learner/reset.py:
                         // the moments restart at zero there, so Adam's step count does); null = 0
};

__host__ __device__ inline int opt_mode(const OptSched& s) {
  return s.adam ? OPT_ADAM : (s.ctr != nullptr ? OPT_RMSPROP_SCHED : OPT_RMSPROP);
}

// Soft (Polyak) target network, Runtime.target_ema_rate = rho: the launch that has just
// formed the updated weight p' also writes
//   t' = fl(fl(a t) + fl(rho p')),  a = fl(1 - rho)   (fp32, no contraction: rho = 1 gives p' exactly)
// in every format the forward reads the target net in: the fp32 master copy, the bf16 hi
// (/ lo) planes and, in the peeled first chunk, the target halves of the fused forward's
// fragment buffers.  learner/schedules.py target_ema is the host mirror, bit for bit.
struct OptTarget {
  float* t;             // fp32 target parameters (null: off)
  bf16_t* tb;           // their bf16 copy
  bf16_t* tb_lo;        // its lo plane (split mode: set exactly when RmspropArgs.pb_lo is)
  float rho;
  CfFragOut tfo;        // the fused forward's TARGET operands in fragment order (w1frag null: off)
};

struct RmspropArgs {
  float* p;
  const float* g;
  float* v;
  float* m;
  bf16_t* pb;
  int64_t n;
  const double* partials;
  int npart;
  float lr, alpha, eps, clip;
  int centered;
  float* norm_out;
  bf16_t* pb_lo;     // fp32-accurate mode: lo plane of the bf16 copy (p = pb + pb_lo), else null
  const double* wnorm;  // batch-max IS normalisation (is_grad_scale), or null
  int wn, wstride;
  CfFragOut fo;         // the fused forward's online operands in fragment order (w1frag null: off)
  const float* gpre;    // clip norm: a gradient range summed in every block (clip_coef_from_partials), or null
  int64_t npre;
  OptSched os;          // update index + schedules + Adam constants (all-zero: OPT_RMSPROP)
  OptTarget tg;         // soft target net averaged in the same launch (t null: off, the EMA = false code)
};

// one block `bid` of `nblk` (grid-stride over float4 chunks)
// EMA: the launch also averages the target net (OptTarget); every difference is an
// `if constexpr`, so the EMA = false instantiations are the code of before
template <int MODE = OPT_RMSPROP, bool EMA = false>
__device__ __forceinline__ void rmsprop_body(const RmspropArgs& A_, int bid, int nblk) {
  // no FMA contraction: every inlined copy of the update (steady loop, peeled chunk, the
  // other launches) rounds identically
#pragma clang fp contract(off)
  float* __restrict__ p = A_.p;
  const float* __restrict__ g = A_.g;
  float* __restrict__ v = A_.v;
  float* __restrict__ m = A_.m;
  bf16_t* __restrict__ pb = A_.pb;
  bf16_t* __restrict__ pbl = A_.pb_lo;
  const int64_t n = A_.n;
  const float alpha = MODE == OPT_ADAM ? (float)A_.os.beta2 : A_.alpha, eps = A_.eps;
  const int centered = MODE == OPT_ADAM ? 1 : A_.centered;    // (Adam: m is the first moment)
  // sh[0], sh[1]: clip coefficient and norm; the scheduled variants add sh[2] = lr(u),
  // sh[3] = 1 - beta1^t, sh[4] = 1 - beta2^t, written by thread 0 ahead of the clip
  // reduction's barriers
  __shared__ float sh[MODE == OPT_RMSPROP ? 2 : 5];
  const int64_t n4 = n / 4;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* v4 = reinterpret_cast<float4*>(v);
  float4* m4 = reinterpret_cast<float4*>(m);
  uint2* pb4 = reinterpret_cast<uint2*>(pb);
  uint2* pbl4 = reinterpret_cast<uint2*>(pbl);
  float* __restrict__ t = nullptr;
  bf16_t* __restrict__ tb = nullptr;
  bf16_t* __restrict__ tbl = nullptr;
  float4* t4 = nullptr;
  uint2* tb4 = nullptr;
  uint2* tbl4 = nullptr;
  float rho = 0.f, arho = 0.f;
  if constexpr (EMA) {
    t = A_.tg.t; tb = A_.tg.tb; tbl = A_.tg.tb_lo;
    t4 = reinterpret_cast<float4*>(t);
    tb4 = reinterpret_cast<uint2*>(tb);
    tbl4 = reinterpret_cast<uint2*>(tbl);
    rho = A_.tg.rho;
    arho = 1.0f - rho;
  }
  const int64_t stride = (int64_t)nblk * blockDim.x;
  int64_t i = (int64_t)bid * blockDim.x + threadIdx.x;
  // the first chunk's loads are in flight while the block sums the clip-norm
  // partials, and every iteration prefetches the next chunk (one-deep pipeline)
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gg = z4, pp = z4, vv = z4, mm = z4, tt = z4;
  if (i < n4) {
    gg = g4[i]; pp = p4[i]; vv = v4[i];
    if (centered) mm = m4[i];
    if constexpr (EMA) tt = t4[i];
  }
  if constexpr (MODE != OPT_RMSPROP) {
    if (threadIdx.x == 0) {
      const OptSched& os = A_.os;
      int64_t u = (int64_t)os.ctr[0] - os.base[0] - 1;
      u = u < 0 ? 0 : u;
      sh[2] = sched_lr(u, os.lr0, os.lr_end, os.warmup, os.decay);
      if constexpr (MODE == OPT_ADAM) {
        int64_t t = u + 1 - (os.t0 != nullptr ? os.t0[0] : 0);
        t = t < 1 ? 1 : t;
        sh[3] = (float)(1.0 - pow_u64(os.beta1, (uint64_t)t));
        sh[4] = (float)(1.0 - pow_u64(os.beta2, (uint64_t)t));
      }
    }
  }
  const float coef = clip_coef_from_partials(A_.partials, A_.npart, A_.clip, sh,
                                             is_grad_scale(A_.wnorm, A_.wn, A_.wstride), A_.gpre, A_.npre);
  if (bid == 0 && threadIdx.x == 0 && A_.norm_out) A_.norm_out[0] = sh[1];
  float lr = A_.lr, c1 = 1.0f, c2 = 1.0f, b1 = 0.f, d1 = 0.f;
  if constexpr (MODE != OPT_RMSPROP) lr = sh[2];
  if constexpr (MODE == OPT_ADAM) {
    c1 = sh[3];
    c2 = sh[4];
    b1 = (float)A_.os.beta1;
    d1 = 1.0f - b1;
  }
  const float a1 = 1.0f - alpha;
  auto update = [&](int64_t i, const float4 gg, const float4 pp, const float4 vv, const float4 mm, const float4 tt,
                    const bool frag) {
    float gx[4] = {gg.x * coef, gg.y * coef, gg.z * coef, gg.w * coef};
    float px[4] = {pp.x, pp.y, pp.z, pp.w};
    float vx[4] = {vv.x, vv.y, vv.z, vv.w};
    float mx[4] = {mm.x, mm.y, mm.z, mm.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (MODE == OPT_ADAM) {
        // m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  p -= lr (m / c1) / (sqrt(v / c2) + eps)
        mx[j] = b1 * mx[j] + d1 * gx[j];
        vx[j] = alpha * vx[j] + a1 * gx[j] * gx[j];
        px[j] -= lr * (mx[j] / c1) / (sqrtf(vx[j] / c2) + eps);
      } else {
        vx[j] = alpha * vx[j] + a1 * gx[j] * gx[j];
        float var = vx[j];
        if (centered) {
          mx[j] = alpha * mx[j] + a1 * gx[j];
          var = vx[j] - mx[j] * mx[j];
        }
        px[j] -= lr * gx[j] / (sqrtf(fmaxf(var, 0.f)) + eps);
      }
    }
    p4[i] = make_float4(px[0], px[1], px[2], px[3]);
    v4[i] = make_float4(vx[0], vx[1], vx[2], vx[3]);
    if (centered) m4[i] = make_float4(mx[0], mx[1], mx[2], mx[3]);
    if (pbl != nullptr) {
      uint32_t h01, l01, h23, l23;
      split_pk_bf16_h(px[0], px[1], h01, l01);
      split_pk_bf16_h(px[2], px[3], h23, l23);
      pb4[i] = make_uint2(h01, h23);
      pbl4[i] = make_uint2(l01, l23);
      if (frag) cf_frag_store(A_.fo, 4 * i, px, make_uint2(h01, h23), make_uint2(l01, l23));
    } else {
      const uint2 hb = make_uint2(pack_bf16x2(px[0], px[1]), pack_bf16x2(px[2], px[3]));
      pb4[i] = hb;
      if (frag) cf_frag_store(A_.fo, 4 * i, px, hb, make_uint2(0u, 0u));
    }
    if constexpr (EMA) {
      // the target net from the weights just written: two products and a sum, each rounded
      float tx[4] = {tt.x, tt.y, tt.z, tt.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ta = arho * tx[j], pr = rho * px[j];
        tx[j] = ta + pr;
      }
      t4[i] = make_float4(tx[0], tx[1], tx[2], tx[3]);
      const bool tfrag = frag && A_.tg.tfo.w1frag != nullptr;
      if (tbl != nullptr) {
        uint32_t h01, l01, h23, l23;
        split_pk_bf16_h(tx[0], tx[1], h01, l01);
        split_pk_bf16_h(tx[2], tx[3], h23, l23);
        tb4[i] = make_uint2(h01, h23);
        tbl4[i] = make_uint2(l01, l23);
        if (tfrag) cf_frag_store(A_.tg.tfo, 4 * i, tx, make_uint2(h01, h23), make_uint2(l01, l23));
      } else {
        const uint2 hb = make_uint2(pack_bf16x2(tx[0], tx[1]), pack_bf16x2(tx[2], tx[3]));
        tb4[i] = hb;
        if (tfrag) cf_frag_store(A_.tg.tfo, 4 * i, tx, hb, make_uint2(0u, 0u));
      }
    }
  };
  // The first chunk is peeled: the fused forward's operand stores (A_.fo, the launcher
  // checks that w1 / w2 lie within every thread's first chunk) run before the next
  // chunk's loads are issued, so the steady loop keeps 6 waves per SIMD (every block of
  // the launch resident at once; with the stores inside the loop it held 85 VGPRs).
  // That is the RMSprop instantiations' figure (74 / 75 VGPRs); OPT_ADAM's three divisions
  // per element hold 86 / 87 VGPRs, 5 waves per SIMD -- the fused launch's 256 blocks of 8
  // waves are one per CU either way
  if (i < n4) {
    update(i, gg, pp, vv, mm, tt, A_.fo.w1frag != nullptr);     // (the launcher: tg.tfo only beside fo)
    i += stride;
    if (i < n4) {
      gg = g4[i]; pp = p4[i]; vv = v4[i];
      if (centered) mm = m4[i];
      if constexpr (EMA) tt = t4[i];
    }
  }
  for (; i < n4; i += stride) {
    const int64_t inx = i + stride;
    float4 gn = z4, pn = z4, vn = z4, mn = z4, tn = z4;
    if (inx < n4) {
      gn = g4[inx]; pn = p4[inx]; vn = v4[inx];
      if (centered) mn = m4[inx];
      if constexpr (EMA) tn = t4[inx];
    }
    update(i, gg, pp, vv, mm, tt, false);
    gg = gn; pp = pn; vv = vn; mm = mn;
    if constexpr (EMA) tt = tn;
  }
  for (int64_t i = n4 * 4 + (int64_t)bid * blockDim.x + threadIdx.x; i < n; i += (int64_t)nblk * blockDim.x) {
    float gg = g[i] * coef;
    float vv = alpha * v[i] + a1 * gg * gg, var = vv;
    v[i] = vv;
    float pp;
    if constexpr (MODE == OPT_ADAM) {
      const float mm = b1 * m[i] + d1 * gg;
      m[i] = mm;
      pp = p[i] - lr * (mm / c1) / (sqrtf(vv / c2) + eps);
    } else {
      if (centered) {
        float mm = alpha * m[i] + a1 * gg;
        m[i] = mm;
        var = vv - mm * mm;
      }
      pp = p[i] - lr * gg / (sqrtf(fmaxf(var, 0.f)) + eps);
    }
    p[i] = pp;
    pb[i] = f32_to_bf16(pp);
    if (pbl != nullptr) pbl[i] = f32_to_bf16(pp - bf16_to_f32(pb[i]));
    if constexpr (EMA) {
      const float ta = arho * t[i], pr = rho * pp;
      const float tn = ta + pr;
      t[i] = tn;
      tb[i] = f32_to_bf16(tn);
      if (tbl != nullptr) tbl[i] = f32_to_bf16(tn - bf16_to_f32(tb[i]));
    }
  }
}

// Launcher-side checks of an optimizer launch's target block against its online arguments
// (`first`: the elements every thread's first chunk covers, the range cf_frag_store runs in;
// `n0`: the elements of the range that holds the fragment sources).  0 = fine.
inline int opt_target_check(const OptTarget& g, const bf16_t* pb_lo, const CfFragOut& fo, int64_t n0, int64_t first) {
  if (g.t == nullptr) return (g.tb != nullptr || g.tb_lo != nullptr || g.tfo.w1frag != nullptr) ? 1 : 0;
  if (g.tb == nullptr || (g.tb_lo != nullptr) != (pb_lo != nullptr) || !(g.rho >= 0.f && g.rho <= 1.f)) return 1;
  if (((uintptr_t)g.t & 15) || (((uintptr_t)g.tb | (uintptr_t)g.tb_lo) & 7)) return 1;
  const CfFragOut& f = g.tfo;
  if (f.w1frag == nullptr) return 0;
  // the target fragments go where the online ones do: same offsets, same first-chunk rule
  if (fo.w1frag == nullptr || f.c2f == nullptr || f.C != fo.C || f.w1_off != fo.w1_off || f.w2_off != fo.w2_off ||
      (f.c3f != nullptr) != (fo.c3f != nullptr) || (f.c3f != nullptr && f.w3_off != fo.w3_off) ||
      f.in_scale != fo.in_scale)
    return 1;
  if ((f.C != 1 && f.C != 2 && f.C != 4) || (f.w1_off & 3) || (f.w2_off & 7) || f.w1_off + 4096LL * f.C > n0 ||
      f.w2_off + 65536 > n0 || f.w1_off + 4096LL * f.C > first || f.w2_off + 65536 > first ||
      (((uintptr_t)f.w1frag | (uintptr_t)f.c2f) & 15))
    return 1;
  if (f.c3f != nullptr && ((f.w3_off & 3) || f.w3_off + 36864 > n0 || f.w3_off + 36864 > first || ((uintptr_t)f.c3f & 15)))
    return 1;
  return 0;
}

// The checks every optimizer launch form makes (`n0`, `first`: as opt_target_check): the float4 / packed-bf16
// alignment of the flat arrays, a step-indexed mode's counter and base, and the target block.
inline bool opt_args_ok(const RmspropArgs& a, int64_t n0, int64_t first) {
  if (((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.v | (uintptr_t)a.m) & 15) return false;
  if (((uintptr_t)a.pb | (uintptr_t)a.pb_lo) & 7) return false;
  if (opt_mode(a.os) != OPT_RMSPROP && (a.os.ctr == nullptr || a.os.base == nullptr)) return false;
  if (a.os.t0 != nullptr && (opt_mode(a.os) != OPT_ADAM || ((uintptr_t)a.os.t0 & 7))) return false;
  return opt_target_check(a.tg, a.pb_lo, a.fo, n0, first) == 0;
}

// f(mode, ema) with the block's MODE and EMA as integral constants: the one MODE x EMA ladder of the launchers
template <class F>
inline void opt_dispatch(const RmspropArgs& a, F&& f) {
  auto with_ema = [&](auto ema) {
    const int mode = opt_mode(a.os);
    if (mode == OPT_ADAM) f(std::integral_constant<int, OPT_ADAM>{}, ema);
    else if (mode == OPT_RMSPROP_SCHED) f(std::integral_constant<int, OPT_RMSPROP_SCHED>{}, ema);
    else f(std::integral_constant<int, OPT_RMSPROP>{}, ema);
  };
  if (a.tg.t != nullptr) with_ema(std::true_type{});
  else with_ema(std::false_type{});
}
