// Periodic shrink-and-perturb reset of the flat parameter vector (Runtime.reset_interval; learner/reset.py is
// the host mirror and the definition): for element i of table row s and reset number r
//
//   k      = apex_u24(seed_r, r, i)
//   phi_i  = fp32((double)(2 k + 1 - 2^24) / 2^24 * (double)bound_s)      (0 on nature32's padding; a sigma row: its constant)
//   p'_i   = fl(fl(alpha_s p_i) + fl(fl(1 - alpha_s) phi_i)),  t'_i the same on the target with the same phi_i
//   v_i = m_i = 0
//
//   reset_perturb_kernel   one launch over the flat vector in float4 chunks (grid-stride).  The table (at most 32
//                          rows, one per segment) is copied from the arguments into LDS; every chunk finds its row
//                          by a search over it and chunks in an alignment gap return.  Rows start on a chunk boundary
//                          (the launcher checks), so a chunk never straddles two rows; the one chunk that straddles
//                          a row's END stores its leading elements one by one and leaves the gap untouched.  Writes
//                          p32, t32, zeros in rms_v / rms_m, and both nets' bf16 hi plane (lo plane in split mode)
//                          with the optimizer's packing helpers.  Plain vector stores, no atomics, no scratch.
//
// It runs eagerly between graph replays, once per reset_interval updates: a bandwidth pass, not tuned beyond 16-B accesses.
#include "apex_common.h"

#define RESET_MAX_ROWS 32     // learner/reset.py MAX_ROWS

struct ResetRow {
  int64_t start, end;    // flat element range [start, end)
  int64_t period, live;  // element i is drawn iff (i - start) % period < live, else phi = 0
  float bound, alpha;
  int const_flag;        // 1: const_value in the place of phi (the noisy layers' sigma)
  float const_value;
};

struct ResetArgs {
  float* p;              // fp32 online parameters
  float* t;              // fp32 target parameters
  float* v;              // optimizer moments
  float* m;
  bf16_t* pb;            // bf16 hi planes of both nets
  bf16_t* tb;
  bf16_t* pb_lo;         // split mode: their lo planes (both or neither)
  bf16_t* tb_lo;
  int64_t n;             // elements of every flat array
  uint64_t seed;         // seed_r (learner/reset.py reset_seed)
  uint64_t r;            // reset number, from 1
  int nrows;
  ResetRow rows[RESET_MAX_ROWS];
};

// one element: (p', t') of (p, t)
__device__ __forceinline__ void reset_elem(const ResetRow& w, uint64_t seed, uint64_t r, int64_t i, float al, float be,
                                           float& p, float& t) {
#pragma clang fp contract(off)
  float phi;
  if (w.const_flag) {
    phi = w.const_value;
  } else if (w.live < w.period && (uint32_t)(i - w.start) % (uint32_t)w.period >= (uint32_t)w.live) {
    phi = 0.f;
  } else {
    const int32_t k = (int32_t)apex_u24(seed, r, (uint64_t)i);
    phi = (float)((double)(2 * k + 1 - (1 << 24)) / 16777216.0 * (double)w.bound);
  }
  const float f = be * phi;
  const float pa = al * p, ta = al * t;
  p = pa + f;
  t = ta + f;
}

__global__ void __launch_bounds__(256) reset_perturb_kernel(ResetArgs a) {
#pragma clang fp contract(off)
  __shared__ ResetRow s_rows[RESET_MAX_ROWS];
  if ((int)threadIdx.x < a.nrows) s_rows[threadIdx.x] = a.rows[threadIdx.x];
  __syncthreads();
  const int nrows = a.nrows;
  const int64_t n4 = a.n / 4;
  float4* p4 = reinterpret_cast<float4*>(a.p);
  float4* t4 = reinterpret_cast<float4*>(a.t);
  float4* v4 = reinterpret_cast<float4*>(a.v);
  float4* m4 = reinterpret_cast<float4*>(a.m);
  uint2* pb4 = reinterpret_cast<uint2*>(a.pb);
  uint2* tb4 = reinterpret_cast<uint2*>(a.tb);
  uint2* pbl4 = reinterpret_cast<uint2*>(a.pb_lo);
  uint2* tbl4 = reinterpret_cast<uint2*>(a.tb_lo);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n4; c += stride) {
    const int64_t i0 = 4 * c;
    int row = -1;
    for (int k = 0; k < nrows; ++k)
      if (i0 >= s_rows[k].start && i0 < s_rows[k].end) row = k;
    if (row < 0) continue;       // an alignment gap
    const ResetRow& w = s_rows[row];
    const float al = w.alpha, be = 1.0f - al;
    if (i0 + 4 <= w.end) {
      const float4 pp = p4[c], tt = t4[c];
      float px[4] = {pp.x, pp.y, pp.z, pp.w};
      float tx[4] = {tt.x, tt.y, tt.z, tt.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) reset_elem(w, a.seed, a.r, i0 + j, al, be, px[j], tx[j]);
      p4[c] = make_float4(px[0], px[1], px[2], px[3]);
      t4[c] = make_float4(tx[0], tx[1], tx[2], tx[3]);
      v4[c] = z4;
      m4[c] = z4;
      if (pbl4 != nullptr) {
        uint32_t h01, l01, h23, l23;
        split_pk_bf16_h(px[0], px[1], h01, l01);
        split_pk_bf16_h(px[2], px[3], h23, l23);
        pb4[c] = make_uint2(h01, h23);
        pbl4[c] = make_uint2(l01, l23);
        split_pk_bf16_h(tx[0], tx[1], h01, l01);
        split_pk_bf16_h(tx[2], tx[3], h23, l23);
        tb4[c] = make_uint2(h01, h23);
        tbl4[c] = make_uint2(l01, l23);
      } else {
        pb4[c] = make_uint2(pack_bf16x2(px[0], px[1]), pack_bf16x2(px[2], px[3]));
        tb4[c] = make_uint2(pack_bf16x2(tx[0], tx[1]), pack_bf16x2(tx[2], tx[3]));
      }
    } else {
      // the row ends inside this chunk: its elements one by one, the gap behind them untouched
      for (int64_t i = i0; i < w.end; ++i) {
        float pp = a.p[i], tt = a.t[i];
        reset_elem(w, a.seed, a.r, i, al, be, pp, tt);
        a.p[i] = pp;
        a.t[i] = tt;
        a.v[i] = 0.f;
        a.m[i] = 0.f;
        const bf16_t ph = f32_to_bf16(pp), th = f32_to_bf16(tt);
        a.pb[i] = ph;
        a.tb[i] = th;
        if (a.pb_lo != nullptr) {
          a.pb_lo[i] = f32_to_bf16(pp - bf16_to_f32(ph));
          a.tb_lo[i] = f32_to_bf16(tt - bf16_to_f32(th));
        }
      }
    }
  }
}

// The launcher's checks (host): the float4 / packed-bf16 alignment of the flat arrays, a target block consistent
// with the online one (lo planes: both or neither), and a table of 1..32 ordered, non-overlapping rows that start
// on a chunk boundary and end inside [0, n).
inline bool reset_args_ok(const ResetArgs& a) {
  if (a.p == nullptr || a.t == nullptr || a.v == nullptr || a.m == nullptr || a.pb == nullptr || a.tb == nullptr)
    return false;
  if (((uintptr_t)a.p | (uintptr_t)a.t | (uintptr_t)a.v | (uintptr_t)a.m) & 15) return false;
  if (((uintptr_t)a.pb | (uintptr_t)a.tb | (uintptr_t)a.pb_lo | (uintptr_t)a.tb_lo) & 7) return false;
  if ((a.pb_lo != nullptr) != (a.tb_lo != nullptr)) return false;
  if (a.n < 4 || (a.n & 3) || a.n >= (1ll << 31)) return false;
  if (a.nrows < 1 || a.nrows > RESET_MAX_ROWS) return false;
  int64_t prev = 0;
  for (int k = 0; k < a.nrows; ++k) {
    const ResetRow& w = a.rows[k];
    if ((w.start & 3) || w.start < prev || w.end <= w.start || w.end > a.n) return false;
    if (w.period < 1 || w.live < 0 || w.live > w.period) return false;
    if (!(w.alpha >= 0.f && w.alpha <= 1.f) || !(w.bound >= 0.f && w.bound <= 1.f)) return false;
    if (w.const_flag != 0 && w.const_flag != 1) return false;
    prev = w.end;
  }
  return true;
}

// Refuses (no launch) what reset_args_ok refuses.
APEX_EXPORT int apex_reset_perturb(ResetArgs a, hipStream_t st) {
  if (!reset_args_ok(a)) return (int)hipErrorInvalidValue;
  const int64_t n4 = a.n / 4;
  int64_t blocks = (n4 + 255) / 256;
  blocks = blocks > 2048 ? 2048 : blocks;
  reset_perturb_kernel<<<(unsigned)blocks, 256, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}

APEX_EXPORT int apex_reset_args_size() { return (int)sizeof(ResetArgs); }
