// LayerNorm on the two 3136 -> 512 stream layers of the dueling NatureCNN (Runtime.layer_norm), between the
// Linear and the ReLU (torch's nn.LayerNorm(512): biased variance, per-feature affine).  For a forward row and
// stream s in {value, advantage}, a = W x + b the fc pre-activation:
//
//   mu = (1/512) sum a_i      d_i = a_i - mu      v = (1/512) sum d_i^2        (two passes, never E[a^2] - mu^2)
//   r = 1 / sqrt(v + eps)     xh_i = d_i r        z_i = gamma_i xh_i + beta_i  h_i = max(z_i, 0)
//
// and backward, dz the head's dH (already zero where h = 0):
//
//   g_i = gamma_i dz_i    s1 = (1/512) sum g_i    s2 = (1/512) sum g_i xh_i    da_i = r (g_i - s1 - xh_i s2)
//   G[gamma]_i = sum_b dz_bi xh_bi                G[beta]_i = sum_b dz_bi
//
// Three kernels:
//   fc_ln_epilogue_kernel      in the place of fc_splitk_epilogue_kernel (csrc/conv_mfma.hip): sums the fc GEMM's
//                              split-K partial planes, bias, the normalisation, ReLU, the hi (+ lo) planes of h;
//                              for the training rows also xh and r for the backward
//   fc_ln_bwd_kernel           dH -> da in place, and per row chunk the partial sums of G[gamma], G[beta]
//   fc_ln_wgrad_reduce_kernel  the chunk partials, in chunk order, into G
//
// One wave owns one (row, stream) pair: lane l holds the 8 columns 512 s + 8 l .. + 7 in registers from the loads
// to the stores, and the row sums are xor butterflies over the 64 lanes (every lane ends with the same bits).
// Every sum has one fixed order: the forward's planes in increasing z, the per-lane eight as a balanced tree
// (so a row of identical values has mu = the value exactly and xh = 0), the backward's rows in row order, the
// waves of a block in wave order, the chunks in chunk order.  No float atomics.
#include "conv2_wfrag.h"
#include "mfma_common.h"

#define LN_F 512            // features of one stream
#define LN_COLS 1024        // both streams of a row
#define LN_CHUNK 8          // rows of one backward block (compile time: the results do not depend on the grid)

// the parameter set of a row range: the stream layers' bias, gamma and beta, [value 512 | advantage 512]
struct FcLnSet {
  const float* bias;
  const float* gamma;
  const float* beta;
};

struct FcLnEpiArgs {
  const float* ws;        // [nz][M][1024] fp32 partial planes of the fc GEMM
  int64_t zstride;        // M * 1024
  int nz;
  int M;
  int features;           // 2 x 512
  int m_switch;           // rows >= m_switch take set[1] (M: one set)
  float in_scale;
  float eps;
  FcLnSet set[2];
  bf16_t* y;              // h, hi plane [M][ldy]
  bf16_t* y_lo;           // lo plane (split mode) or null
  int ldy;
  int save_n;             // rows < save_n also leave xh and r
  float* xhat;            // [save_n][1024]
  float* rstd;            // [save_n][2]
  C2dPackJob pk;          // conv2 weight-fragment pack in blocks past the epilogue grid (out = null: none)
};

struct FcLnBwdArgs {
  bf16_t* dH;             // [B][1024] hi plane: dz in, da out
  bf16_t* dH_lo;          // lo plane (split mode) or null
  const float* xhat;      // [B][1024]
  const float* rstd;      // [B][2]
  const float* gamma;     // [1024]
  int B;
  int features;           // 2 x 512
  float* part;            // [chunks][2][1024]: per chunk (sum dz xh | sum dz)
  int64_t part_elems;
  float* g_gamma;         // [1024]
  float* g_beta;          // [1024]
};

// what a launcher refuses, by argument (apex_fc_ln_status_name)
enum FcLnStatus {
  LN_OK = 0, LN_FEATURES = 9001, LN_WS, LN_PARAMS, LN_Y, LN_Y_LO, LN_LDY, LN_SAVE_N, LN_XHAT, LN_RSTD, LN_ROWS,
  LN_M_SWITCH, LN_NZ, LN_PACK, LN_DH, LN_DH_LO, LN_GAMMA, LN_PART, LN_GRAD, LN_STATUS_END
};

static const char* const kLnNames[] = {"features", "ws", "set (bias / gamma / beta)", "y", "y_lo", "ldy", "save_n",
                                       "xhat", "rstd", "rows (M / B)", "m_switch", "nz", "pk", "dH", "dH_lo",
                                       "gamma", "part", "g_gamma / g_beta"};

APEX_EXPORT const char* apex_fc_ln_status_name(int status) {
  if (status < LN_FEATURES || status >= LN_STATUS_END) return nullptr;
  return kLnNames[status - LN_FEATURES];
}

APEX_EXPORT int apex_fc_ln_chunk() { return LN_CHUNK; }
APEX_EXPORT int apex_fc_ln_args_size(int which) {
  return which == 0 ? (int)sizeof(FcLnEpiArgs) : (int)sizeof(FcLnBwdArgs);
}

__device__ __forceinline__ void ln_load8(const float* __restrict__ p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ void ln_store8(float* __restrict__ p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// the lane's eight as a balanced tree, then the xor butterfly: 512 identical values sum exactly
__device__ __forceinline__ float ln_tree8(const float (&v)[8]) {
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

__device__ __forceinline__ float ln_butterfly(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// packed bf16 pairs of one 16-byte load -> fp32
__device__ __forceinline__ void ln_unpack8(const uint4 u, float (&v)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[2 * q] = __uint_as_float(w[q] << 16);
    v[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
  }
}

// fp32 x 8 -> the hi (+ lo) planes, one 16-byte store per plane
template <bool SPLIT>
__device__ __forceinline__ void ln_store_planes(bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int64_t off,
                                                const float (&v)[8]) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (SPLIT) split_pk_bf16(v[2 * q], v[2 * q + 1], h[q], l[q]);
    else h[q] = cvt_pk_bf16(v[2 * q], v[2 * q + 1]);
  }
  *reinterpret_cast<uint4*>(hi + off) = make_uint4(h[0], h[1], h[2], h[3]);
  if (SPLIT) *reinterpret_cast<uint4*>(lo + off) = make_uint4(l[0], l[1], l[2], l[3]);
}

// ---------------------------------------------------------------------------------------------- forward
// grid: eb = ceil(2 M / 4) blocks of four (row, stream) waves, then the pack job's blocks.
template <bool SPLIT>
__global__ void __launch_bounds__(256) fc_ln_epilogue_kernel(FcLnEpiArgs a, int eb) {
  if ((int)blockIdx.x >= eb) {
    pack_c2d_wfrag_word(((int)blockIdx.x - eb) * 256 + threadIdx.x, a.pk.w, a.pk.w_lo, a.pk.out);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int pair = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int m = pair >> 1, s = pair & 1;
  if (m >= a.M) return;                       // (wave-uniform; no barrier in this kernel)
  const int col = LN_F * s + 8 * lane;
  const int64_t e = (int64_t)m * LN_COLS + col;

  float v[8];
  ln_load8(a.ws + e, v);
  for (int z = 1; z < a.nz; ++z) {
    float p[8];
    ln_load8(a.ws + (int64_t)z * a.zstride + e, p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += p[i];
  }
  const bool second = m >= a.m_switch;         // (wave-uniform: scalar selects of the kernel arguments)
  float b[8], gm[8], bt[8];
  ln_load8((second ? a.set[1].bias : a.set[0].bias) + col, b);
  ln_load8((second ? a.set[1].gamma : a.set[0].gamma) + col, gm);
  ln_load8((second ? a.set[1].beta : a.set[0].beta) + col, bt);
  // a: the value the plain epilogue would have ReLU'd
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = v[i] * a.in_scale + b[i];

  const float mu = ln_butterfly(ln_tree8(v)) * (1.0f / LN_F);
  float d2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] -= mu;
    d2[i] = v[i] * v[i];
  }
  const float var = ln_butterfly(ln_tree8(d2)) * (1.0f / LN_F);
  // fp64 on the fp32 inputs, rounded to fp32 once (the convention of csrc/value_rescale.h)
  const float r = (float)(1.0 / sqrt((double)var + (double)a.eps));
  float h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] *= r;                                 // xh
    h[i] = fmaxf(gm[i] * v[i] + bt[i], 0.f);
  }
  ln_store_planes<SPLIT>(a.y, a.y_lo, (int64_t)m * a.ldy + col, h);
  if (m < a.save_n) {
    ln_store8(a.xhat + e, v);
    if (lane == 0) a.rstd[2 * m + s] = r;
  }
}

static int fc_ln_epi_check(const FcLnEpiArgs& a) {
  if (a.features != LN_COLS) return LN_FEATURES;
  if (a.M < 1 || (int64_t)a.M * LN_COLS >= (1ll << 31)) return LN_ROWS;
  if (a.nz < 1 || a.nz > 64 || a.zstride < (int64_t)a.M * LN_COLS) return LN_NZ;
  if (a.ws == nullptr || ((uintptr_t)a.ws & 15) || (a.zstride & 3)) return LN_WS;
  if (a.m_switch < 0 || a.m_switch > a.M) return LN_M_SWITCH;
  for (int k = 0; k < 2; ++k) {
    const FcLnSet& p = a.set[k];
    if (k == 1 && a.m_switch == a.M) break;   // (one set: the second is not read)
    if (p.bias == nullptr || p.gamma == nullptr || p.beta == nullptr) return LN_PARAMS;
    if (((uintptr_t)p.bias | (uintptr_t)p.gamma | (uintptr_t)p.beta) & 15) return LN_PARAMS;
  }
  if (a.y == nullptr || ((uintptr_t)a.y & 15)) return LN_Y;
  if ((uintptr_t)a.y_lo & 15) return LN_Y_LO;
  if (a.ldy < LN_COLS || (a.ldy & 7)) return LN_LDY;
  if (a.save_n < 0 || a.save_n > a.M) return LN_SAVE_N;
  if (a.save_n > 0 && (a.xhat == nullptr || ((uintptr_t)a.xhat & 15))) return LN_XHAT;
  if (a.save_n > 0 && (a.rstd == nullptr || ((uintptr_t)a.rstd & 3))) return LN_RSTD;
  if (a.pk.out != nullptr && (a.pk.w == nullptr || ((uintptr_t)a.pk.out & 15))) return LN_PACK;
  return LN_OK;
}

// Refuses (no launch, the status names the argument: apex_fc_ln_status_name) what fc_ln_epi_check refuses.
APEX_EXPORT int apex_fc_ln_epilogue(FcLnEpiArgs a, hipStream_t st) {
  const int bad = fc_ln_epi_check(a);
  if (bad) return bad;
  const int eb = (2 * a.M + 3) / 4;
  const int pb = a.pk.out != nullptr ? C2D_PACK_THREADS / 256 : 0;
  if (a.y_lo != nullptr) fc_ln_epilogue_kernel<true><<<eb + pb, 256, 0, st>>>(a, eb);
  else fc_ln_epilogue_kernel<false><<<eb + pb, 256, 0, st>>>(a, eb);
  APEX_CHECK_LAUNCH();
}

// --------------------------------------------------------------------------------------------- backward
// grid (chunks, 2 streams): the four waves walk the chunk's rows, wave w the rows w, w + 4, ...
template <bool SPLIT>
__global__ void __launch_bounds__(256) fc_ln_bwd_kernel(FcLnBwdArgs a) {
  __shared__ float red[4][2][LN_F];            // (wave, sum dz xh | sum dz, column)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int row0 = (int)blockIdx.x * LN_CHUNK;
  const int col = LN_F * s + 8 * lane;
  float gm[8];
  ln_load8(a.gamma + col, gm);
  float acc_g[8], acc_b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc_g[i] = acc_b[i] = 0.f;

#pragma unroll
  for (int k = wv; k < LN_CHUNK; k += 4) {
    const int m = row0 + k;
    if (m >= a.B) break;                       // (wave-uniform; the barrier is below the loop)
    const int64_t e = (int64_t)m * LN_COLS + col;
    float dz[8], xh[8];
    ln_unpack8(*reinterpret_cast<const uint4*>(a.dH + e), dz);
    if (SPLIT) {
      float lo[8];
      ln_unpack8(*reinterpret_cast<const uint4*>(a.dH_lo + e), lo);
#pragma unroll
      for (int i = 0; i < 8; ++i) dz[i] += lo[i];
    }
    ln_load8(a.xhat + e, xh);
    const float r = a.rstd[2 * m + s];
    float g[8], gx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      g[i] = gm[i] * dz[i];
      gx[i] = g[i] * xh[i];
    }
    // s1 and s2 as one two-value butterfly
    float t1 = ln_tree8(g), t2 = ln_tree8(gx);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      t1 += __shfl_xor(t1, o, 64);
      t2 += __shfl_xor(t2, o, 64);
    }
    const float s1 = t1 * (1.0f / LN_F), s2 = t2 * (1.0f / LN_F);
    float da[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      da[i] = r * (g[i] - s1 - xh[i] * s2);
      acc_g[i] += dz[i] * xh[i];
      acc_b[i] += dz[i];
    }
    ln_store_planes<SPLIT>(a.dH, a.dH_lo, e, da);
  }

  ln_store8(&red[wv][0][8 * lane], acc_g);
  ln_store8(&red[wv][1][8 * lane], acc_b);
  __syncthreads();
  // thread t: four columns of one of the two sums, the waves in wave order
  const int which = threadIdx.x >> 7, c4 = (threadIdx.x & 127) * 4;
  float4 t = *reinterpret_cast<const float4*>(&red[0][which][c4]);
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float4 u = *reinterpret_cast<const float4*>(&red[w][which][c4]);
    t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
  }
  *reinterpret_cast<float4*>(a.part + ((int64_t)blockIdx.x * 2 + which) * LN_COLS + LN_F * s + c4) = t;
}

// G[gamma], G[beta] = the chunk planes added in chunk order: one thread per column of one sum, so the 2 x 1024
// columns spread over eight blocks (a wave reads 256 contiguous bytes of a plane).
__global__ void __launch_bounds__(256) fc_ln_wgrad_reduce_kernel(const float* __restrict__ part, int chunks,
                                                                 float* __restrict__ g_gamma,
                                                                 float* __restrict__ g_beta) {
  const int t = (int)blockIdx.x * 256 + threadIdx.x;      // (sum, column)
  if (t >= 2 * LN_COLS) return;
  const int which = t / LN_COLS, col = t - which * LN_COLS;
  // 16 planes' loads in flight at a time (one dependent load per plane made this launch 19 us at 64 chunks),
  // the adds still in chunk order
  float acc = 0.f;
  for (int c0 = 0; c0 < chunks; c0 += 16) {
    float u[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) u[k] = c0 + k < chunks ? part[((int64_t)(c0 + k) * 2 + which) * LN_COLS + col] : 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc += u[k];
  }
  (which ? g_beta : g_gamma)[col] = acc;
}

static int fc_ln_bwd_check(const FcLnBwdArgs& a) {
  if (a.features != LN_COLS) return LN_FEATURES;
  if (a.B < 1 || (int64_t)a.B * LN_COLS >= (1ll << 31)) return LN_ROWS;
  if (a.dH == nullptr || ((uintptr_t)a.dH & 15)) return LN_DH;
  if ((uintptr_t)a.dH_lo & 15) return LN_DH_LO;
  if (a.xhat == nullptr || ((uintptr_t)a.xhat & 15)) return LN_XHAT;
  if (a.rstd == nullptr || ((uintptr_t)a.rstd & 3)) return LN_RSTD;
  if (a.gamma == nullptr || ((uintptr_t)a.gamma & 15)) return LN_GAMMA;
  const int64_t chunks = (a.B + LN_CHUNK - 1) / LN_CHUNK;
  if (a.part == nullptr || ((uintptr_t)a.part & 15) || a.part_elems < chunks * 2 * LN_COLS) return LN_PART;
  return LN_OK;
}

// da in place over dH (+ dH_lo) and the chunk partials.  Refuses what fc_ln_bwd_check refuses.
APEX_EXPORT int apex_fc_ln_bwd(FcLnBwdArgs a, hipStream_t st) {
  const int bad = fc_ln_bwd_check(a);
  if (bad) return bad;
  const dim3 grid((a.B + LN_CHUNK - 1) / LN_CHUNK, 2);
  if (a.dH_lo != nullptr) fc_ln_bwd_kernel<true><<<grid, 256, 0, st>>>(a);
  else fc_ln_bwd_kernel<false><<<grid, 256, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}

// The chunk partials of the last apex_fc_ln_bwd with the same arguments -> g_gamma, g_beta (overwritten).
APEX_EXPORT int apex_fc_ln_wgrad_reduce(FcLnBwdArgs a, hipStream_t st) {
  const int bad = fc_ln_bwd_check(a);
  if (bad) return bad;
  if (a.g_gamma == nullptr || a.g_beta == nullptr || (((uintptr_t)a.g_gamma | (uintptr_t)a.g_beta) & 15))
    return LN_GRAD;
  fc_ln_wgrad_reduce_kernel<<<2 * LN_COLS / 256, 256, 0, st>>>(a.part, (a.B + LN_CHUNK - 1) / LN_CHUNK, a.g_gamma, a.g_beta);
  APEX_CHECK_LAUNCH();
}
