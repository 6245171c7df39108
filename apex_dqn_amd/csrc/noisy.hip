// Factorised NoisyNet fc and head layers (Fortunato et al. 2018) for the fused NatureCNN
// learner and the GPU actors (learner/noisy.py is the host mirror and the definition).
//
//   noisy_compose_kernel      W = mu + sigma * (xi_out (x) xi_in), b = mu_b + sigma_b * xi_out
//                             of the fc layer and the two heads, for one or two networks in
//                             one launch (grid.y = net), written into shadow buffers of the
//                             mu layout in the formats the forward / backward kernels read:
//                             fp32 for the head weights and every noisy bias, the bf16 hi
//                             plane (+ the lo plane in split mode) for wfc.
//   noisy_sigma_grad_kernel   G[sigma] = G[mu] * xi_out (x) xi_in from the online draw, once
//                             the gradients w.r.t. the effective weights are final.
//
// The draw index u is read from device memory (the replay's draw counter minus the
// learner's base word: updates completed, read at the head of an update, rmsprop_common.h;
// an actor group's call counter), so a replayed graph draws fresh noise with no host round
// trip.  Every block recomputes the xi it needs (its columns' xi_in into LDS, its rows'
// xi_out): 3136 + 4 counter-RNG evaluations beside 12.5 K streamed elements, and no second
// launch or grid-wide hand-off in front of a bandwidth-bound pass.  The first block of each
// part also writes its xi to the draw buffer, which the sigma-gradient kernel and the tests
// read.
//
// Each effective value is formed in fp64 (xi_out * xi_in is exact there) and rounded once to
// fp32: within half an ulp (plus fp64 rounding) of the exact value, whatever mu and the
// noise term cancel to.  The hi / lo planes are the project's split of that fp32 value
// (apex_common.h split_pk_bf16_h, the optimizer's and cast_bf16's).
#include "apex_common.h"

#define NZ_FC_IN 3136
#define NZ_FC_OUT 1024
#define NZ_HID 512
#define NZ_FC_RT 4   // fc rows per block: 256 blocks per net
#define NZ_HD_RT 8   // head rows per block
#define NZ_STREAMS 64

struct NoisyNet {
  const float* p;   // flat parameters: mu and sigma segments
  float* e32;       // fp32 shadow (mu layout): head weights and the noisy biases
  bf16_t* ehi;      // bf16 shadow (mu layout): wfc hi plane
  bf16_t* elo;      // its lo plane (split mode), or null
  float* fc32;      // fp32 effective wfc [1024][3136] (tests), or null
  float* xi;        // the draw, K floats
};

struct NoisyArgs {
  NoisyNet net[2];
  int nnets, A, N, stream0;
  int64_t mu[6];    // flat offsets of wv, bv, wa, ba, wfc, bfc
  int64_t sg[6];    // and of their sigma segments
  uint64_t seed;
  const uint64_t* ctr;
  const int64_t* base;  // or null
  int64_t every;
  int64_t n_p, n_e;     // lengths of p and of the shadows (launcher checks)
};

struct NoisyGradArgs {
  float* g;
  const float* xi;
  int A, N;
  int64_t mu[6], sg[6];
  int64_t n_g;
};

enum { NZ_WV = 0, NZ_BV, NZ_WA, NZ_BA, NZ_WFC, NZ_BFC };

// offsets of the seven parts of the concatenated draw (learner/noisy.py xi_offsets)
struct XiOff {
  int fc_out, v_in, a_in, v_out, a_out, K;
};
__host__ __device__ inline XiOff xi_off(int A, int N) {
  XiOff o;
  o.fc_out = 2 * NZ_FC_IN;
  o.v_in = o.fc_out + NZ_FC_OUT;
  o.a_in = o.v_in + NZ_HID;
  o.v_out = o.a_in + NZ_HID;
  o.a_out = o.v_out + N;
  o.K = o.a_out + A * N;
  return o;
}

// xi = sign(g) sqrt(|g|), g = sqrt(-2 ln u1) cos(2 pi u2) from the counter RNG's uniforms.
// Accurate logf / sqrtf / cospif (no fast-math variants): the mirror evaluates g in fp64.
__device__ __forceinline__ float noisy_xi(uint64_t seed, uint64_t c, uint32_t k) {
  const float u1 = 1.0f - apex_uniform(seed, c, 2ull * k);        // (0, 1], exact
  const float u2 = apex_uniform(seed, c, 2ull * k + 1ull);
  const float g = sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
  return copysignf(sqrtf(fabsf(g)), g);
}

__device__ __forceinline__ float noisy_eff(float mu, float sg, float xo, float xin) {
  return (float)((double)mu + (double)sg * ((double)xo * (double)xin));
}

__global__ void __launch_bounds__(256) noisy_compose_kernel(NoisyArgs a) {
  __shared__ __attribute__((aligned(16))) float s_in[NZ_FC_IN];
  __shared__ float s_out[NZ_HD_RT];
  const int nid = blockIdx.y, tid = threadIdx.x;
  const NoisyNet nt = a.net[nid];
  int64_t u = (int64_t)a.ctr[0] - (a.base != nullptr ? a.base[0] : 0);
  u = (u < 0 ? 0 : u) / a.every;
  const uint64_t c = (uint64_t)NZ_STREAMS * (uint64_t)u + (uint64_t)(a.stream0 + nid);
  const XiOff xo = xi_off(a.A, a.N);
  const int fc_tiles = NZ_FC_OUT / NZ_FC_RT;
  int t = blockIdx.x;
  if (t < fc_tiles) {
    const int r0 = t * NZ_FC_RT;
    const int k_in = r0 >= NZ_HID ? NZ_FC_IN : 0;       // value / advantage stream
    const bool first = (r0 & (NZ_HID - 1)) == 0;
    for (int j = tid; j < NZ_FC_IN; j += 256) {
      const float x = noisy_xi(a.seed, c, (uint32_t)(k_in + j));
      s_in[j] = x;
      if (first) nt.xi[k_in + j] = x;
    }
    if (tid < NZ_FC_RT) {
      const int r = r0 + tid;
      const float x = noisy_xi(a.seed, c, (uint32_t)(xo.fc_out + r));
      s_out[tid] = x;
      nt.xi[xo.fc_out + r] = x;
      nt.e32[a.mu[NZ_BFC] + r] = noisy_eff(nt.p[a.mu[NZ_BFC] + r], nt.p[a.sg[NZ_BFC] + r], x, 1.0f);
    }
    __syncthreads();
    const float* __restrict__ pm = nt.p + a.mu[NZ_WFC];
    const float* __restrict__ ps = nt.p + a.sg[NZ_WFC];
    constexpr int CH = NZ_FC_IN / 8;   // 16-B bf16 chunks per row
    for (int q = tid; q < NZ_FC_RT * CH; q += 256) {
      const int row = q / CH, col = (q - row * CH) * 8;
      const int64_t idx = (int64_t)(r0 + row) * NZ_FC_IN + col;
      const float4 m0 = *reinterpret_cast<const float4*>(pm + idx);
      const float4 m1 = *reinterpret_cast<const float4*>(pm + idx + 4);
      const float4 g0 = *reinterpret_cast<const float4*>(ps + idx);
      const float4 g1 = *reinterpret_cast<const float4*>(ps + idx + 4);
      const float4 x0 = *reinterpret_cast<const float4*>(s_in + col);
      const float4 x1 = *reinterpret_cast<const float4*>(s_in + col + 4);
      const float o = s_out[row];
      float w[8];
      w[0] = noisy_eff(m0.x, g0.x, o, x0.x); w[1] = noisy_eff(m0.y, g0.y, o, x0.y);
      w[2] = noisy_eff(m0.z, g0.z, o, x0.z); w[3] = noisy_eff(m0.w, g0.w, o, x0.w);
      w[4] = noisy_eff(m1.x, g1.x, o, x1.x); w[5] = noisy_eff(m1.y, g1.y, o, x1.y);
      w[6] = noisy_eff(m1.z, g1.z, o, x1.z); w[7] = noisy_eff(m1.w, g1.w, o, x1.w);
      uint4 hi, lo;
      if (nt.elo != nullptr) {
        split_pk_bf16_h(w[0], w[1], hi.x, lo.x);
        split_pk_bf16_h(w[2], w[3], hi.y, lo.y);
        split_pk_bf16_h(w[4], w[5], hi.z, lo.z);
        split_pk_bf16_h(w[6], w[7], hi.w, lo.w);
        *reinterpret_cast<uint4*>(nt.elo + a.mu[NZ_WFC] + idx) = lo;
      } else {
        hi = make_uint4(pack_bf16x2(w[0], w[1]), pack_bf16x2(w[2], w[3]), pack_bf16x2(w[4], w[5]),
                        pack_bf16x2(w[6], w[7]));
      }
      *reinterpret_cast<uint4*>(nt.ehi + a.mu[NZ_WFC] + idx) = hi;
      if (nt.fc32 != nullptr) {
        *reinterpret_cast<float4*>(nt.fc32 + idx) = make_float4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<float4*>(nt.fc32 + idx + 4) = make_float4(w[4], w[5], w[6], w[7]);
      }
    }
    return;
  }
  // the heads: fp32 only
  t -= fc_tiles;
  const int v_tiles = (a.N + NZ_HD_RT - 1) / NZ_HD_RT;
  const bool adv = t >= v_tiles;
  if (adv) t -= v_tiles;
  const int rows = adv ? a.A * a.N : a.N;
  const int r0 = t * NZ_HD_RT;
  const int k_in = adv ? xo.a_in : xo.v_in, k_out = adv ? xo.a_out : xo.v_out;
  const int64_t ow = a.mu[adv ? NZ_WA : NZ_WV], ob = a.mu[adv ? NZ_BA : NZ_BV];
  const int64_t sw = a.sg[adv ? NZ_WA : NZ_WV], sb = a.sg[adv ? NZ_BA : NZ_BV];
  for (int j = tid; j < NZ_HID; j += 256) {
    const float x = noisy_xi(a.seed, c, (uint32_t)(k_in + j));
    s_in[j] = x;
    if (t == 0) nt.xi[k_in + j] = x;
  }
  if (tid < NZ_HD_RT && r0 + tid < rows) {
    const int r = r0 + tid;
    const float x = noisy_xi(a.seed, c, (uint32_t)(k_out + r));
    s_out[tid] = x;
    nt.xi[k_out + r] = x;
    nt.e32[ob + r] = noisy_eff(nt.p[ob + r], nt.p[sb + r], x, 1.0f);
  }
  __syncthreads();
  constexpr int CH4 = NZ_HID / 4;
  for (int q = tid; q < NZ_HD_RT * CH4; q += 256) {
    const int row = q / CH4, col = (q - row * CH4) * 4;
    if (r0 + row >= rows) break;
    const int64_t idx = (int64_t)(r0 + row) * NZ_HID + col;
    const float4 m = *reinterpret_cast<const float4*>(nt.p + ow + idx);
    const float4 g = *reinterpret_cast<const float4*>(nt.p + sw + idx);
    const float4 x = *reinterpret_cast<const float4*>(s_in + col);
    const float o = s_out[row];
    *reinterpret_cast<float4*>(nt.e32 + ow + idx) =
        make_float4(noisy_eff(m.x, g.x, o, x.x), noisy_eff(m.y, g.y, o, x.y), noisy_eff(m.z, g.z, o, x.z),
                    noisy_eff(m.w, g.w, o, x.w));
  }
}

__device__ __forceinline__ float noisy_sg(float g, float xo, float xin) {
  return (float)((double)g * ((double)xo * (double)xin));
}

__global__ void __launch_bounds__(256) noisy_sigma_grad_kernel(NoisyGradArgs a) {
  const int tid = threadIdx.x;
  const XiOff xo = xi_off(a.A, a.N);
  const int fc_tiles = NZ_FC_OUT / NZ_FC_RT;
  int t = blockIdx.x;
  if (t < fc_tiles) {
    const int r0 = t * NZ_FC_RT;
    const float* __restrict__ xin = a.xi + (r0 >= NZ_HID ? NZ_FC_IN : 0);
    const float* __restrict__ gm = a.g + a.mu[NZ_WFC];
    float* __restrict__ gs = a.g + a.sg[NZ_WFC];
    if (tid < NZ_FC_RT) {
      const int r = r0 + tid;
      a.g[a.sg[NZ_BFC] + r] = noisy_sg(a.g[a.mu[NZ_BFC] + r], a.xi[xo.fc_out + r], 1.0f);
    }
    constexpr int CH4 = NZ_FC_IN / 4;
    for (int q = tid; q < NZ_FC_RT * CH4; q += 256) {
      const int row = q / CH4, col = (q - row * CH4) * 4;
      const int64_t idx = (int64_t)(r0 + row) * NZ_FC_IN + col;
      const float4 g = *reinterpret_cast<const float4*>(gm + idx);
      const float4 x = *reinterpret_cast<const float4*>(xin + col);
      const float o = a.xi[xo.fc_out + r0 + row];
      *reinterpret_cast<float4*>(gs + idx) =
          make_float4(noisy_sg(g.x, o, x.x), noisy_sg(g.y, o, x.y), noisy_sg(g.z, o, x.z), noisy_sg(g.w, o, x.w));
    }
    return;
  }
  t -= fc_tiles;
  const int v_tiles = (a.N + NZ_HD_RT - 1) / NZ_HD_RT;
  const bool adv = t >= v_tiles;
  if (adv) t -= v_tiles;
  const int rows = adv ? a.A * a.N : a.N;
  const int r0 = t * NZ_HD_RT;
  const float* __restrict__ xin = a.xi + (adv ? xo.a_in : xo.v_in);
  const float* __restrict__ xout = a.xi + (adv ? xo.a_out : xo.v_out);
  const int64_t ow = a.mu[adv ? NZ_WA : NZ_WV], ob = a.mu[adv ? NZ_BA : NZ_BV];
  const int64_t sw = a.sg[adv ? NZ_WA : NZ_WV], sb = a.sg[adv ? NZ_BA : NZ_BV];
  if (tid < NZ_HD_RT && r0 + tid < rows) {
    const int r = r0 + tid;
    a.g[sb + r] = noisy_sg(a.g[ob + r], xout[r], 1.0f);
  }
  constexpr int CH4 = NZ_HID / 4;
  for (int q = tid; q < NZ_HD_RT * CH4; q += 256) {
    const int row = q / CH4, col = (q - row * CH4) * 4;
    if (r0 + row >= rows) break;
    const int64_t idx = (int64_t)(r0 + row) * NZ_HID + col;
    const float4 g = *reinterpret_cast<const float4*>(a.g + ow + idx);
    const float4 x = *reinterpret_cast<const float4*>(xin + col);
    const float o = xout[r0 + row];
    *reinterpret_cast<float4*>(a.g + sw + idx) =
        make_float4(noisy_sg(g.x, o, x.x), noisy_sg(g.y, o, x.y), noisy_sg(g.z, o, x.z), noisy_sg(g.w, o, x.w));
  }
}

// every segment inside its buffer, 16-B aligned where the kernels use 16-B accesses
static bool noisy_layout_ok(const int64_t* mu, const int64_t* sg, int A, int N, int64_t n_mu, int64_t n_sg) {
  if (A < 1 || N < 1 || (int64_t)A * N > (1 << 20)) return false;
  const int64_t len[6] = {(int64_t)N * NZ_HID, N, (int64_t)A * N * NZ_HID, (int64_t)A * N,
                          (int64_t)NZ_FC_OUT * NZ_FC_IN, NZ_FC_OUT};
  for (int i = 0; i < 6; ++i) {
    if (mu[i] < 0 || sg[i] < 0 || mu[i] + len[i] > n_mu || sg[i] + len[i] > n_sg) return false;
    if (len[i] >= NZ_HID && ((mu[i] | sg[i]) & 7)) return false;      // weights: 16-B (bf16: 8 elements)
  }
  return true;
}

static int noisy_tiles(int A, int N) {
  return NZ_FC_OUT / NZ_FC_RT + (N + NZ_HD_RT - 1) / NZ_HD_RT + (A * N + NZ_HD_RT - 1) / NZ_HD_RT;
}

APEX_EXPORT int apex_noisy_xi_len(int A, int N) { return xi_off(A, N).K; }

APEX_EXPORT int apex_noisy_compose(NoisyArgs a, hipStream_t st) {
  if (a.nnets < 1 || a.nnets > 2 || a.ctr == nullptr || a.every < 1 || a.stream0 < 0 ||
      a.stream0 + a.nnets > NZ_STREAMS)
    return (int)hipErrorInvalidValue;
  if (!noisy_layout_ok(a.mu, a.sg, a.A, a.N, a.n_e < a.n_p ? a.n_e : a.n_p, a.n_p)) return (int)hipErrorInvalidValue;
  for (int i = 0; i < a.nnets; ++i) {
    const NoisyNet& n = a.net[i];
    if (n.p == nullptr || n.e32 == nullptr || n.ehi == nullptr || n.xi == nullptr) return (int)hipErrorInvalidValue;
    if (((uintptr_t)n.p | (uintptr_t)n.e32 | (uintptr_t)n.ehi | (uintptr_t)n.elo | (uintptr_t)n.fc32) & 15)
      return (int)hipErrorInvalidValue;
  }
  noisy_compose_kernel<<<dim3((unsigned)noisy_tiles(a.A, a.N), (unsigned)a.nnets), 256, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}

APEX_EXPORT int apex_noisy_sigma_grad(NoisyGradArgs a, hipStream_t st) {
  if (a.g == nullptr || a.xi == nullptr || (((uintptr_t)a.g | (uintptr_t)a.xi) & 15)) return (int)hipErrorInvalidValue;
  if (!noisy_layout_ok(a.mu, a.sg, a.A, a.N, a.n_g, a.n_g)) return (int)hipErrorInvalidValue;
  noisy_sigma_grad_kernel<<<noisy_tiles(a.A, a.N), 256, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}
