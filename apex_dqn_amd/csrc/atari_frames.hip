// Raw Atari frames -> the replay's space-to-depth frame ring, in one kernel:
// max over the two raw 210x160x3 frames of an env step, gray, area resize to 84x84, rounding,
// the [21][21][4][4] byte permutation and the ring scatter (with wrap).
//
// The arithmetic is exact integer math, so the result has one right answer that the host mirror
// (envs/vector_envs.py atari_preprocess_exact) reproduces bit for bit:
//   m   = max(frame0, frame1) per byte
//   g   = 299 R + 587 G + 114 B                                   (<= 255 000)
//   rows 210 -> 84 (scale 5/2): even output row 2k takes input rows 5k, 5k+1, 5k+2 with weights
//        2, 2, 1; odd row 2k+1 takes 5k+2, 5k+3, 5k+4 with weights 1, 2, 2   (sum 5)
//   cols 160 -> 84 (scale 40/21): output column j covers [40j, 40j+40) in units of 1/21 input
//        pixel, input column c covers [21c, 21c+21); the weight is the overlap (<= 3 taps, sum 40)
//   out = acc / 200000 rounded half to even, acc = sum w_r w_c g <= 51 000 000 (int32)
//
// Work item = (frame pair f, s2d block row R): output rows 4R..4R+3 need exactly input rows
// 10R..10R+9 -- 4800 contiguous bytes of each raw frame -- and fill 336 contiguous bytes of the
// ring slot (21 blocks of 16 B).  One 256-thread workgroup per item:
//   1. 16-B coalesced loads of both bands, bytewise max, ds_write_b128 into LDS;
//   2. gray + row pass: one thread per (column, band half), int32 row sums into LDS;
//   3. column pass + rounding: one thread per output pixel, bytes into LDS in s2d order;
//   4. lanes 0..20 store one 16-B s2d block each.
#include "apex_common.h"

namespace {

constexpr int AF_THREADS = 256;
constexpr int AF_W = 160;                       // raw frame width
constexpr int AF_ROW_BYTES = AF_W * 3;          // 480
constexpr int AF_FRAME_BYTES = 210 * AF_ROW_BYTES;   // 100 800
constexpr int AF_BAND_V4 = 10 * AF_ROW_BYTES / 16;   // 300 uint4 per 10-row band
constexpr int AF_SLOT_BYTES = 84 * 84;          // 7056
constexpr int AF_OUT_V4 = 21;                   // s2d blocks per block row

typedef unsigned short af_u16x2 __attribute__((ext_vector_type(2)));

// max of four packed bytes: even and odd bytes as two u16 lanes each (v_pk_max_u16)
__device__ __forceinline__ uint32_t af_max_u8x4(uint32_t a, uint32_t b) {
  const uint32_t m = 0x00ff00ffu;
  const af_u16x2 e = __builtin_elementwise_max(__builtin_bit_cast(af_u16x2, a & m), __builtin_bit_cast(af_u16x2, b & m));
  const af_u16x2 o = __builtin_elementwise_max(__builtin_bit_cast(af_u16x2, (a >> 8) & m),
                                               __builtin_bit_cast(af_u16x2, (b >> 8) & m));
  return __builtin_bit_cast(uint32_t, e) | (__builtin_bit_cast(uint32_t, o) << 8);
}

__global__ __launch_bounds__(AF_THREADS) void atari_frames_kernel(const uint8_t* __restrict__ raw,
                                                                  uint8_t* __restrict__ ring, int64_t F,
                                                                  int64_t start) {
  __shared__ uint4 band[AF_BAND_V4];            // max of the two frames' rows 10R..10R+9, RGB bytes
  __shared__ int rowp[4][AF_W];                 // row pass: 5 x area-weighted gray per output row
  __shared__ uint4 outv[AF_OUT_V4];             // 4 x 84 output bytes in s2d order
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x / 21;
  const int R = blockIdx.x - (int)f * 21;

  const uint4* s0 = reinterpret_cast<const uint4*>(raw + f * (2 * (int64_t)AF_FRAME_BYTES) + R * (10 * AF_ROW_BYTES));
  const uint4* s1 = s0 + AF_FRAME_BYTES / 16;
  for (int i = tid; i < AF_BAND_V4; i += AF_THREADS) {
    const uint4 a = s0[i], b = s1[i];
    band[i] = make_uint4(af_max_u8x4(a.x, b.x), af_max_u8x4(a.y, b.y), af_max_u8x4(a.z, b.z), af_max_u8x4(a.w, b.w));
  }
  __syncthreads();

  const uint8_t* px = reinterpret_cast<const uint8_t*>(band);
  for (int i = tid; i < 2 * AF_W; i += AF_THREADS) {
    const int h = i / AF_W, c = i - h * AF_W;   // band half h: input rows 5h..5h+4 -> output rows 2h, 2h+1
    const uint8_t* p = px + (5 * h) * AF_ROW_BYTES + 3 * c;
    int g[5];
#pragma unroll
    for (int r = 0; r < 5; ++r)
      g[r] = 299 * p[r * AF_ROW_BYTES] + 587 * p[r * AF_ROW_BYTES + 1] + 114 * p[r * AF_ROW_BYTES + 2];
    rowp[2 * h][c] = 2 * g[0] + 2 * g[1] + g[2];
    rowp[2 * h + 1][c] = g[2] + 2 * g[3] + 2 * g[4];
  }
  __syncthreads();

  uint8_t* ob = reinterpret_cast<uint8_t*>(outv);
  for (int i = tid; i < 4 * 84; i += AF_THREADS) {
    const int j = i / 84, x = i - j * 84;       // output row 4R + j, column x
    const int lo = 40 * x, hi = lo + 40;
    const int c0 = lo / 21;
    int acc = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int c = c0 + t;
      const int w = min(hi, 21 * c + 21) - max(lo, 21 * c);   // overlap; <= 0 past the last tap
      acc += max(w, 0) * rowp[j][min(c, AF_W - 1)];
    }
    int q = acc / 200000;
    const int r2 = 2 * (acc - q * 200000);
    q += (r2 > 200000 || (r2 == 200000 && (q & 1))) ? 1 : 0;
    ob[(x >> 2) * 16 + j * 4 + (x & 3)] = (uint8_t)q;
  }
  __syncthreads();

  if (tid < AF_OUT_V4) {
    uint8_t* o = ring + ((start + f) % F) * AF_SLOT_BYTES + R * (AF_OUT_V4 * 16) + tid * 16;
    *reinterpret_cast<uint4*>(o) = outv[tid];
  }
}

}  // namespace

// raw [n][2][210][160][3] uint8 -> ring slots (start + f) % F, f = 0..n-1, each [21][21][4][4].
// n <= F: two frames of one call never share a slot (the caller keeps only the newest F).
APEX_EXPORT int apex_atari_frames(const uint8_t* raw, uint8_t* ring, int64_t n, int64_t F, int64_t start,
                                  hipStream_t st) {
  if (n <= 0) return 0;
  if (raw == nullptr || ring == nullptr || ((uintptr_t)raw & 15) || ((uintptr_t)ring & 15))
    return (int)hipErrorInvalidValue;
  if (F <= 0 || n > F || start < 0 || start >= F || n > (int64_t)0x7fffffff / 21) return (int)hipErrorInvalidValue;
  atari_frames_kernel<<<(int)(n * 21), AF_THREADS, 0, st>>>(raw, ring, F, start);
  APEX_CHECK_LAUNCH();
}
