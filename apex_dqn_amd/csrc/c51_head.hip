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
//
// c51_head_kernel: one block of C51_NT threads per C51_SPB samples, three phases.
//   1. The 3 C51_SPB activation rows (online S_t, online S_t+n, target S_t+n; hi + lo in
//      split mode) are staged in LDS as fp32.  Every wave takes weight rows four at a time:
//      16 lanes per row, lane l of them columns 64 c + 4 l .. + 3 (c = 0..7) as eight
//      float4 loads -- each load instruction reads four 256-B runs -- multiplies them with
//      every staged row of that weight set (ds_read_b128, the four 16-lane groups read the
//      same addresses) and reduces within its 16 lanes by four DPP steps.  A block reads
//      both weight sets once for C51_SPB samples; the next group's weights are loaded
//      while the current one is multiplied.
//   2. Wave s finishes sample s with lane = atom: softmax per action, expectations, a*, the
//      projection (p'_j and b_j by lane shuffles), loss, priority and the dhead row, which
//      it also leaves in LDS.
//   3. dH for the block's samples: the threads form four groups of 128, a thread holds
//      four columns, group q adds rows q, q + 4, .. of dhead . W (float4 weight loads, the
//      coefficients broadcast from LDS); the groups' partials are added through LDS in a
//      fixed order.  The weights are read once more per block.
// Nothing depends on the order blocks run in (no float atomics).
//
// c51_actor_head_kernel: one wave per env row, the logits as in phase 1 with the row in
// registers, then the expected q per action and the epsilon-greedy draw of
// actor_head_kernel (same counter-RNG words).
#include "head_common.h"

#define C51_SPB 2      // samples per block
#define C51_NT 512     // 8 waves
#define C51_HS 512

struct C51Args {
  const bf16_t* Hon;    // [2B][2 HS]
  const bf16_t* Htg;    // [B][2 HS]
  HeadParams Pon, Ptg;
  const int32_t* act;
  const float* rew;
  const float* gam;
  const float* isw;     // null: weights off
  int B, A, N, hidden;
  float vmin, vmax, grad_scale;
  float* td_abs;
  float* loss;
  float* q_out;         // [B][A] expected q(S_t), or null
  bf16_t* dH;           // [B][2 HS]
  float* dhead;         // [B][(A + 1) N]
  float* zero_ptr;      // head-gradient region zeroed for the head weight gradient
  int zero_n;
  HeadLo lo;
  IsNorm isn;
};

// sum over each 16-lane row (every lane of the row holds it)
__device__ __forceinline__ float row16_sum(float v) {
  APEX_DPP_ADD(v, 0xB1);   // quad_perm(1,0,3,2)
  APEX_DPP_ADD(v, 0x4E);   // quad_perm(2,3,0,1)
  APEX_DPP_ADD(v, 0x124);  // row_ror:4
  APEX_DPP_ADD(v, 0x128);  // row_ror:8
  return v;
}

// the 8 float4 of weight row `wrow` this lane multiplies (columns 64 c + 4 l16 ..)
__device__ __forceinline__ void c51_load_w(const float* __restrict__ wrow, int l16, float4* w) {
#pragma unroll
  for (int c = 0; c < 8; ++c) w[c] = *reinterpret_cast<const float4*>(wrow + c * 64 + l16 * 4);
}

__device__ __forceinline__ float c51_dot(const float4* w, const float4* h) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    acc = fmaf(w[c].x, h[c].x, acc);
    acc = fmaf(w[c].y, h[c].y, acc);
    acc = fmaf(w[c].z, h[c].z, acc);
    acc = fmaf(w[c].w, h[c].w, acc);
  }
  return acc;
}

// Weight-row groups of one weight set: [0, gv) value rows, [gv, gv + ga) advantage rows,
// four rows each (the last group of a stream clamps its row; the store skips it).
struct C51Group {
  const float* wrow;   // this lane's weight row
  int soff;            // stream offset of the activations (0 value, HS advantage)
  int j;               // logit column (N + a N + i for advantages), or -1: no store
};

__device__ __forceinline__ C51Group c51_group(const HeadParams& P, int u, int gv, int N, int AN, int lane) {
  C51Group g;
  const int sub = lane >> 4;
  if (u < gv) {
    const int r = u * 4 + sub;
    g.wrow = P.wv + (int64_t)min(r, N - 1) * C51_HS;
    g.soff = 0;
    g.j = r < N ? r : -1;
  } else {
    const int r = (u - gv) * 4 + sub;
    g.wrow = P.wa + (int64_t)min(r, AN - 1) * C51_HS;
    g.soff = C51_HS;
    g.j = r < AN ? N + r : -1;
  }
  return g;
}

// One activation row's distribution terms, lane = atom (valid = lane < N): L = the row's
// logits without biases ([N] value, then [A][N]).
struct C51Row {
  const float* L;
  const float* bv;
  const float* ba;
  float v;      // value logit + bias of this lane's atom
  float mean;   // mean over the actions of (advantage + bias)
};

__device__ __forceinline__ C51Row c51_row(const float* L, const HeadParams& P, int A, int N, int lane) {
  C51Row r;
  r.L = L;
  r.bv = P.bv;
  r.ba = P.ba;
  const bool valid = lane < N;
  r.v = valid ? L[lane] + P.bv[lane] : 0.f;
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += valid ? L[N + a * N + lane] + P.ba[a * N + lane] : 0.f;
  r.mean = s / (float)A;
  return r;
}

// softmax over the atoms of action a: this lane's probability and log-probability;
// returns the expectation sum_i p_i z_i (wave-uniform)
__device__ __forceinline__ float c51_action(const C51Row& r, int a, int N, int lane, float z, float& p, float& lp) {
  const bool valid = lane < N;
  const float l = valid ? r.v + (r.L[N + a * N + lane] + r.ba[a * N + lane]) - r.mean : -3.0e38f;
  const float mx = wave_max(l);
  const float e = valid ? expf(l - mx) : 0.f;
  const float Z = wave_sum_dpp(e);
  p = e / Z;
  lp = valid ? (l - mx) - logf(Z) : 0.f;
  return wave_sum_dpp(p * z);
}

__global__ void __launch_bounds__(C51_NT) c51_head_kernel(C51Args a) {
  extern __shared__ __attribute__((aligned(16))) float c51_smem[];
  constexpr int HS = C51_HS, ROW = 2 * HS, SPB = C51_SPB, NR = 3 * SPB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int B = a.B, A = a.A, N = a.N, AN = A * N, J = N + AN;
  const int Jp = (J + 3) & ~3;
  float* Hs = c51_smem;                  // [NR][ROW]: rows s (S_t), SPB + s (online S_t+n), 2 SPB + s (target)
  float* Ls = c51_smem + NR * ROW;       // [NR][Jp] logits (no biases); rows s later hold the dhead rows
  const int b0 = blockIdx.x * SPB;
  const bool split = a.lo.Hon != nullptr;

  // zero the head-gradient region that the head weight gradient accumulates into
  if (a.zero_ptr != nullptr)
    for (int i = blockIdx.x * C51_NT + tid; i < a.zero_n; i += gridDim.x * C51_NT) a.zero_ptr[i] = 0.f;
  // batch-max IS statistic (ddqn_head_kernel's): block 0's last wave
  if ((a.isn.out != nullptr || a.isn.valid_count != nullptr) && blockIdx.x == 0 && wv == C51_NT / 64 - 1) {
    float m = 0.f;
    int nv = 0;
    for (int i = lane; i < B; i += 64) {
      m = fmaxf(m, a.isw[i]);
      nv += a.isw[i] > 0.f ? 1 : 0;
    }
    m = wave_max(m);
    nv = wave_sum(nv);
    if (lane == 0) {
      const float ws = a.isn.wscale != nullptr ? a.isn.wscale[0] : 1.f;
      if (a.isn.out != nullptr) a.isn.out[0] = ws > 0.f ? (double)m / (double)ws : 0.0;
      if (a.isn.valid_count != nullptr) atomicAdd(a.isn.valid_count, (unsigned long long)nv);
    }
  }

  // ---- phase 0: the block's activation rows -> LDS (fp32; a sample past the batch reads the last row)
  for (int r = 0; r < NR; ++r) {
    const int s = r % SPB, kind = r / SPB;
    const int b = min(b0 + s, B - 1);
    const int64_t off = (kind == 1 ? (int64_t)(B + b) : (int64_t)b) * ROW;
    const bf16_t* src = (kind == 2 ? a.Htg : a.Hon) + off;
    const uint32_t u = reinterpret_cast<const uint32_t*>(src)[tid];          // columns 2 tid, 2 tid + 1
    float x0 = __uint_as_float(u << 16), x1 = __uint_as_float(u & 0xffff0000u);
    if (split) {
      const bf16_t* sl = (kind == 2 ? a.lo.Htg : a.lo.Hon) + off;
      const uint32_t v = reinterpret_cast<const uint32_t*>(sl)[tid];
      x0 += __uint_as_float(v << 16);
      x1 += __uint_as_float(v & 0xffff0000u);
    }
    *reinterpret_cast<float2*>(Hs + r * ROW + 2 * tid) = make_float2(x0, x1);
  }
  __syncthreads();

  // ---- phase 1: logits of every staged row
  {
    const int l16 = lane & 15;
    const int gv = (N + 3) >> 2, ga = (AN + 3) >> 2, G1 = gv + ga;
    constexpr int NW = C51_NT / 64;
    float4 w[8], wn[8];
    int t = wv;
    C51Group g{a.Pon.wv, 0, -1};
    if (t < 2 * G1) {       // (a tiny head has fewer tasks than waves)
      g = c51_group(t >= G1 ? a.Ptg : a.Pon, t >= G1 ? t - G1 : t, gv, N, AN, lane);
      c51_load_w(g.wrow, l16, w);
    }
    for (; t < 2 * G1; t += NW) {
      const int tn = t + NW;
      C51Group gn = g;
      if (tn < 2 * G1) {
        gn = c51_group(tn >= G1 ? a.Ptg : a.Pon, tn >= G1 ? tn - G1 : tn, gv, N, AN, lane);
        c51_load_w(gn.wrow, l16, wn);
      }
      const bool tg = t >= G1;
      const int r0 = tg ? 2 * SPB : 0, nr = tg ? SPB : 2 * SPB;
      for (int rr = 0; rr < nr; ++rr) {
        const float* hrow = Hs + (r0 + rr) * ROW + g.soff + l16 * 4;
        float4 h[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = *reinterpret_cast<const float4*>(hrow + c * 64);
        const float acc = row16_sum(c51_dot(w, h));
        if (l16 == 0 && g.j >= 0) Ls[(r0 + rr) * Jp + g.j] = acc;
      }
      g = gn;
#pragma unroll
      for (int c = 0; c < 8; ++c) w[c] = wn[c];
    }
  }
  __syncthreads();

  // ---- phase 2: wave s finishes sample s (lane = atom)
  if (wv < SPB) {
    const int s = wv;
    const bool live = b0 + s < B;
    const int b = min(b0 + s, B - 1);
    const bool valid = lane < N;
    const float delta = (a.vmax - a.vmin) / (float)(N - 1);
    const float z = a.vmin + (float)lane * delta;
    const int a_b = a.act[b];
    const float rew_b = a.rew[b], gam_b = a.gam[b];
    const float w_b = a.isw != nullptr ? a.isw[b] : 1.f;
    float p, lp;
    // double DQN: a* from the online net at S_t+n (first maximum wins)
    int astar = 0;
    {
      const C51Row rn = c51_row(Ls + (SPB + s) * Jp, a.Pon, A, N, lane);
      float best = -3.4e38f;
      for (int j = 0; j < A; ++j) {
        const float q = c51_action(rn, j, N, lane, z, p, lp);
        if (q > best) { best = q; astar = j; }
      }
      astar = __builtin_amdgcn_readfirstlane(astar);
    }
    // the target net's distribution of a*, projected onto the support
    float m = 0.f;
    {
      const C51Row rg = c51_row(Ls + (2 * SPB + s) * Jp, a.Ptg, A, N, lane);
      c51_action(rg, astar, N, lane, z, p, lp);
      const float pj = valid ? p : 0.f;
      const float tz = fminf(fmaxf(rew_b + gam_b * z, a.vmin), a.vmax);
      const float bj = (tz - a.vmin) / delta;
      const float fi = (float)lane;
      for (int j = 0; j < N; ++j) {      // increasing j: the oracle's order
        const float pp = __shfl(pj, j, 64), bb = __shfl(bj, j, 64);
        m += pp * fmaxf(0.f, 1.f - fabsf(bb - fi));
      }
      if (!valid) m = 0.f;
    }
    // S_t: expected q of every action, the taken action's distribution
    float p_sa = 0.f, lp_sa = 0.f, q_sa = 0.f;
    {
      const C51Row rt = c51_row(Ls + s * Jp, a.Pon, A, N, lane);
      for (int j = 0; j < A; ++j) {
        const float q = c51_action(rt, j, N, lane, z, p, lp);
        if (a.q_out != nullptr && live && lane == 0) a.q_out[(int64_t)b * A + j] = q;
        if (j == a_b) { p_sa = p; lp_sa = lp; q_sa = q; }
      }
    }
    const float ce = -wave_sum_dpp(m * lp_sa);
    const float em = wave_sum_dpp(m * z);
    const float g = valid ? w_b * (p_sa - m) * a.grad_scale : 0.f;
    if (live && lane == 0) {
      a.td_abs[b] = fabsf(em - q_sa);
      a.loss[b] = w_b * ce;
    }
    // the dhead row: to memory, and into LDS (over the consumed S_t logits) for phase 3
    const float invA = 1.0f / (float)A;
    float* D = Ls + s * Jp;
    float* dh = a.dhead + (int64_t)b * J;
    const float gl = live ? g : 0.f;
    if (valid) {
      D[lane] = gl;
      if (live) dh[lane] = g;
      for (int j = 0; j < A; ++j) {
        const float c = (j == a_b ? 1.f : 0.f) - invA;
        D[N + j * N + lane] = gl * c;
        if (live) dh[N + j * N + lane] = g * c;
      }
    }
  }
  __syncthreads();

  // ---- phase 3: dH[s][k] = relu'(h) sum_j dhead[s][j] W[j][k]
  {
    const int q = tid >> 7, ct = tid & 127;       // row group, column quad
    float4 av[SPB], aa[SPB];
#pragma unroll
    for (int s = 0; s < SPB; ++s) av[s] = aa[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* __restrict__ wvp = a.Pon.wv + ct * 4;
    const float* __restrict__ wap = a.Pon.wa + ct * 4;
#pragma unroll 4
    for (int j = q; j < N; j += 4) {
      const float4 w = *reinterpret_cast<const float4*>(wvp + (int64_t)j * HS);
#pragma unroll
      for (int s = 0; s < SPB; ++s) {
        const float c = Ls[s * Jp + j];
        av[s].x = fmaf(c, w.x, av[s].x); av[s].y = fmaf(c, w.y, av[s].y);
        av[s].z = fmaf(c, w.z, av[s].z); av[s].w = fmaf(c, w.w, av[s].w);
      }
    }
#pragma unroll 4
    for (int j = q; j < AN; j += 4) {
      const float4 w = *reinterpret_cast<const float4*>(wap + (int64_t)j * HS);
#pragma unroll
      for (int s = 0; s < SPB; ++s) {
        const float c = Ls[s * Jp + N + j];
        aa[s].x = fmaf(c, w.x, aa[s].x); aa[s].y = fmaf(c, w.y, aa[s].y);
        aa[s].z = fmaf(c, w.z, aa[s].z); aa[s].w = fmaf(c, w.w, aa[s].w);
      }
    }
    // the four groups' partials, added in a fixed order through the LDS rows of the
    // S_t+n activations (consumed): (0 += 2, 1 += 3), then 0 += 1
    float4* red = reinterpret_cast<float4*>(Hs + SPB * ROW);      // [2][SPB][2][128] float4
    auto slot = [&](int gq, int s, int st) { return red + ((gq * SPB + s) * 2 + st) * 128 + ct; };
    if (q >= 2) {
#pragma unroll
      for (int s = 0; s < SPB; ++s) { *slot(q - 2, s, 0) = av[s]; *slot(q - 2, s, 1) = aa[s]; }
    }
    __syncthreads();
    if (q < 2) {
#pragma unroll
      for (int s = 0; s < SPB; ++s) {
        const float4 x = *slot(q, s, 0), y = *slot(q, s, 1);
        av[s].x += x.x; av[s].y += x.y; av[s].z += x.z; av[s].w += x.w;
        aa[s].x += y.x; aa[s].y += y.y; aa[s].z += y.z; aa[s].w += y.w;
      }
    }
    __syncthreads();
    if (q == 1) {
#pragma unroll
      for (int s = 0; s < SPB; ++s) { *slot(0, s, 0) = av[s]; *slot(0, s, 1) = aa[s]; }
    }
    __syncthreads();
    if (q == 0) {
#pragma unroll
      for (int s = 0; s < SPB; ++s) {
        if (b0 + s >= B) continue;
        const float4 x = *slot(0, s, 0), y = *slot(0, s, 1);
        float d[2][4] = {{av[s].x + x.x, av[s].y + x.y, av[s].z + x.z, av[s].w + x.w},
                         {aa[s].x + y.x, aa[s].y + y.y, aa[s].z + y.z, aa[s].w + y.w}};
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const float4 hx = *reinterpret_cast<const float4*>(Hs + s * ROW + st * HS + ct * 4);
          const float m0 = hx.x > 0.f ? d[st][0] : 0.f, m1 = hx.y > 0.f ? d[st][1] : 0.f;
          const float m2 = hx.z > 0.f ? d[st][2] : 0.f, m3 = hx.w > 0.f ? d[st][3] : 0.f;
          const int64_t o = (int64_t)(b0 + s) * ROW + st * HS + ct * 4;
          if (split) {
            uint32_t h0, l0, h1, l1;
            split_pk_bf16_h(m0, m1, h0, l0);
            split_pk_bf16_h(m2, m3, h1, l1);
            *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(a.lo.dH + o) = make_uint2(l0, l1);
          } else {
            *reinterpret_cast<uint2*>(a.dH + o) = make_uint2(pack_bf16x2(m0, m1), pack_bf16x2(m2, m3));
          }
        }
      }
    }
  }
}

static inline size_t c51_head_lds(int A, int N) {
  const int J = (A + 1) * N, Jp = (J + 3) & ~3;
  return (size_t)(3 * C51_SPB) * (2 * C51_HS + Jp) * sizeof(float);
}

APEX_EXPORT int apex_c51_head(C51Args a, hipStream_t st) {
  if (a.A < 1 || a.A > HEAD_MAXA || a.B < 1 || a.N < 2 || a.N > 64 || a.hidden != C51_HS || !(a.vmin < a.vmax))
    return (int)hipErrorInvalidValue;
  if ((a.isn.out != nullptr || a.isn.valid_count != nullptr) && a.isw == nullptr) return (int)hipErrorInvalidValue;
  if (a.lo.Hon != nullptr && (a.lo.Htg == nullptr || a.lo.dH == nullptr)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)a.Pon.wv | (uintptr_t)a.Pon.wa | (uintptr_t)a.Ptg.wv | (uintptr_t)a.Ptg.wa) & 15)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)a.Hon | (uintptr_t)a.Htg | (uintptr_t)a.dH | (uintptr_t)a.lo.Hon | (uintptr_t)a.lo.Htg |
       (uintptr_t)a.lo.dH) & 7)
    return (int)hipErrorInvalidValue;
  const size_t lds = c51_head_lds(a.A, a.N);
  if (lds > 65536) return (int)hipErrorInvalidValue;     // (A + 1) N <= 1706 logits per row
  const int grid = (a.B + C51_SPB - 1) / C51_SPB;
  c51_head_kernel<<<grid, C51_NT, lds, st>>>(a);
  APEX_CHECK_LAUNCH();
}

// Actor side: expected q of the distributional head + epsilon-greedy, one wave per env row
// (four per block; a wave past E repeats the last row and stores nothing).
__global__ void __launch_bounds__(256) c51_actor_head_kernel(const bf16_t* __restrict__ H, HeadParams P, int E, int A,
                                                             int N, float vmin, float vmax,
                                                             const float* __restrict__ eps, uint64_t seed,
                                                             const uint64_t* __restrict__ ctr,
                                                             float* __restrict__ q_out, int32_t* __restrict__ a_out,
                                                             const bf16_t* __restrict__ H_lo) {
  extern __shared__ __attribute__((aligned(16))) float c51_smem[];
  constexpr int HS = C51_HS, ROW = 2 * HS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l16 = lane & 15;
  const int AN = A * N, J = N + AN, Jp = (J + 3) & ~3;
  const int e_raw = blockIdx.x * 4 + wv;
  const bool live = e_raw < E;
  const int e = min(e_raw, E - 1);
  float* L = c51_smem + wv * Jp;
  // this lane's activations of both streams: columns 64 c + 4 l16 .. + 3
  float4 hv[8], ha[8];
  {
    const bf16_t* row = H + (int64_t)e * ROW + l16 * 4;
    const bf16_t* row_lo = H_lo != nullptr ? H_lo + (int64_t)e * ROW + l16 * 4 : nullptr;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const uint2 u = *reinterpret_cast<const uint2*>(row + st * HS + c * 64);
        float4 x = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                               __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
        if (row_lo != nullptr) {
          const uint2 v = *reinterpret_cast<const uint2*>(row_lo + st * HS + c * 64);
          x.x += __uint_as_float(v.x << 16); x.y += __uint_as_float(v.x & 0xffff0000u);
          x.z += __uint_as_float(v.y << 16); x.w += __uint_as_float(v.y & 0xffff0000u);
        }
        if (st) ha[c] = x;
        else hv[c] = x;
      }
    }
  }
  const int gv = (N + 3) >> 2, ga = (AN + 3) >> 2;
  for (int u = 0; u < gv; ++u) {
    const C51Group g = c51_group(P, u, gv, N, AN, lane);
    float4 w[8];
    c51_load_w(g.wrow, l16, w);
    const float acc = row16_sum(c51_dot(w, hv));
    if (l16 == 0 && g.j >= 0) L[g.j] = acc;
  }
  for (int u = gv; u < gv + ga; ++u) {
    const C51Group g = c51_group(P, u, gv, N, AN, lane);
    float4 w[8];
    c51_load_w(g.wrow, l16, w);
    const float acc = row16_sum(c51_dot(w, ha));
    if (l16 == 0 && g.j >= 0) L[g.j] = acc;
  }
  __syncthreads();
  const float delta = (vmax - vmin) / (float)(N - 1);
  const float z = vmin + (float)lane * delta;
  const C51Row r = c51_row(L, P, A, N, lane);
  int best = 0;
  float bq = -3.4e38f, p, lp;
  for (int j = 0; j < A; ++j) {
    const float q = c51_action(r, j, N, lane, z, p, lp);
    if (q > bq) { bq = q; best = j; }
    if (live && lane == 0) q_out[(int64_t)e * A + j] = q;
  }
  if (live && lane == 0) {
    const uint64_t c = ctr ? ctr[0] : 0;
    const float u = apex_uniform(seed, c, 2 * (uint64_t)e);
    const float rr = apex_uniform(seed, c, 2 * (uint64_t)e + 1);
    int act = best;
    if (u < eps[e]) act = min((int)(rr * (float)A), A - 1);
    a_out[e] = act;
  }
}

APEX_EXPORT int apex_c51_actor_head(const bf16_t* H, HeadParams P, int E, int A, int N, float vmin, float vmax,
                                    const float* eps, uint64_t seed, const uint64_t* ctr, float* q_out,
                                    int32_t* a_out, int hidden, const bf16_t* H_lo, hipStream_t st) {
  if (A < 1 || A > HEAD_MAXA || E < 1 || N < 2 || N > 64 || hidden != C51_HS || !(vmin < vmax))
    return (int)hipErrorInvalidValue;
  if ((((uintptr_t)P.wv | (uintptr_t)P.wa) & 15) || (((uintptr_t)H | (uintptr_t)H_lo) & 7))
    return (int)hipErrorInvalidValue;
  const int J = (A + 1) * N, Jp = (J + 3) & ~3;
  c51_actor_head_kernel<<<(E + 3) / 4, 256, (size_t)4 * Jp * sizeof(float), st>>>(H, P, E, A, N, vmin, vmax, eps, seed, ctr,
                                                                                  q_out, a_out, H_lo);
  APEX_CHECK_LAUNCH();
}
