// Random-shift (DrQ) frame augmentation of the sampled batch (learner/augment.py is the host
// mirror and the definition): every sampled frame stack is padded by P pixels with edge
// replication and cropped back to 84 x 84 at an offset in [0, 2P]^2 drawn per (batch row,
// update), the C frames of a row sharing it.
//
//   augment_shift_kernel   one workgroup per (row, frame): the source frame is staged once in
//                          LDS with 16-B loads (7056 B, the ring's space-to-depth layout
//                          [21][21][4][4]); every thread then assembles 16-B output chunks --
//                          one 4 x 4 cell each -- from LDS and stores them, lane after lane 16 B
//                          apart.  A cell row of four output pixels straddles at most two source
//                          cells of one source row: two dword LDS reads and a funnel shift, with
//                          the edge pixel replicated for cells off the frame.  No byte-wide
//                          global access, no scratch, no atomics.
//
// The update index u is read from device memory (the replay's draw counter minus the learner's
// base word, as noisy.hip reads it), so a replayed graph draws fresh offsets with no host
// round trip.  Every workgroup recomputes its row's two offsets (two counter-RNG evaluations);
// frame 0's first thread also writes them to off_out, which the tests and the metrics read.
#include "apex_common.h"

#define AUG_HW 84
#define AUG_CELLS 21                    // 4 x 4 cells per side
#define AUG_FRAME (AUG_HW * AUG_HW)     // 7056 B = 441 x 16 B
#define AUG_CHUNKS (AUG_CELLS * AUG_CELLS)
#define AUG_MAX_PAD 8
#define AUG_STREAMS 64                  // counter word c = 64 u (learner/noisy.py STREAMS_PER_INDEX)

struct AugArgs {
  const uint8_t* ring;   // F frames, space-to-depth bytes
  int64_t F;
  const int32_t* slots;  // [rows][C] ring slots
  int rows, C, pad;
  uint64_t seed;         // seed_a (learner/augment.py aug_seed)
  const uint64_t* ctr;
  const int64_t* base;   // or null
  uint8_t* out;          // [rows][C] frames in the ring's layout
  int64_t n_out;         // bytes at out (launcher check)
  int32_t* off_out;      // [rows][2]: (o_y, o_x)
};

#ifdef APEX_DEBUG_BOUNDS
__device__ int aug_dbg_count;
__device__ long long aug_dbg_first;
#endif

// the dword of cell `cell` in one source pixel row (`rowp`: that row's dword of cell 0, cells 4
// dwords apart); cells off the frame replicate the edge pixel
__host__ __device__ __forceinline__ uint32_t aug_cell_word(const uint32_t* rowp, int cell) {
  if (cell < 0) return (rowp[0] & 0xffu) * 0x01010101u;
  if (cell >= AUG_CELLS) return (rowp[(AUG_CELLS - 1) * 4] >> 24) * 0x01010101u;
  return rowp[cell * 4];
}

// one 4 x 4 output cell (cy, cx) of a frame shifted by (dy, dx) = (o_y - P, o_x - P) pixels:
// out pixel (y, x) = in pixel (clamp(y + dy), clamp(x + dx)); `f`: the source frame's dwords
__host__ __device__ __forceinline__ uint4 aug_cell(const uint32_t* f, int cy, int cx, int dy, int dx) {
  const int x0 = 4 * cx + dx;        // first source column, may be off the frame
  const int cell0 = x0 >> 2;         // floor: arithmetic shift
  const int sh = (x0 & 3) * 8;
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int sy = 4 * cy + i + dy;
    sy = sy < 0 ? 0 : (sy > AUG_HW - 1 ? AUG_HW - 1 : sy);
    const uint32_t* rowp = f + (sy >> 2) * (AUG_CELLS * 4) + (sy & 3);
    const uint32_t a = aug_cell_word(rowp, cell0), b = aug_cell_word(rowp, cell0 + 1);
    w[i] = (uint32_t)((((uint64_t)b << 32) | (uint64_t)a) >> sh);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(256) augment_shift_kernel(AugArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_f[AUG_FRAME / 4];
  const int tid = threadIdx.x;
  const int f = blockIdx.x;            // r C + c
  const int r = f / a.C;
  int64_t u = (int64_t)a.ctr[0] - (a.base != nullptr ? a.base[0] : 0);
  u = u < 0 ? 0 : u;
  const uint64_t c = (uint64_t)AUG_STREAMS * (uint64_t)u;
  const uint32_t span = 2u * (uint32_t)a.pad + 1u;     // k < 2^24, span <= 17: the product fits 32 bits
  const int oy = (int)((apex_u24(a.seed, c, 2ull * (uint64_t)r) * span) >> 24);
  const int ox = (int)((apex_u24(a.seed, c, 2ull * (uint64_t)r + 1ull) * span) >> 24);
  int32_t s = a.slots[f];
#ifdef APEX_DEBUG_BOUNDS
  if (!(s >= 0 && (int64_t)s < a.F)) {
    if (tid == 0 && atomicAdd(&aug_dbg_count, 1) == 0) aug_dbg_first = (long long)s;
    s = s < 0 ? 0 : (int32_t)(a.F - 1);
  }
#endif
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.ring + (int64_t)s * AUG_FRAME);
  uint4* lds16 = reinterpret_cast<uint4*>(s_f);
  for (int q = tid; q < AUG_CHUNKS; q += 256) lds16[q] = src[q];
  if (tid == 0 && f == r * a.C) {
    a.off_out[2 * r] = oy;
    a.off_out[2 * r + 1] = ox;
  }
  __syncthreads();
  const int dy = oy - a.pad, dx = ox - a.pad;
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(a.out + (int64_t)f * AUG_FRAME);
  for (int q = tid; q < AUG_CHUNKS; q += 256) {
    const int cy = q / AUG_CELLS, cx = q - cy * AUG_CELLS;
    dst[q] = aug_cell(s_f, cy, cx, dy, dx);
  }
}

// Refuses (no launch): null pointers, pad outside 1..8, C outside {1, 2, 4}, an output buffer
// shorter than rows C frames or overlapping the ring, pointers off 16 B.
APEX_EXPORT int apex_augment_shift(AugArgs a, hipStream_t st) {
  if (a.ring == nullptr || a.slots == nullptr || a.ctr == nullptr || a.out == nullptr || a.off_out == nullptr)
    return (int)hipErrorInvalidValue;
  if (a.pad < 1 || a.pad > AUG_MAX_PAD || !(a.C == 1 || a.C == 2 || a.C == 4)) return (int)hipErrorInvalidValue;
  if (a.rows < 1 || a.rows > (1 << 24) || a.F < 1) return (int)hipErrorInvalidValue;
  const int64_t need = (int64_t)a.rows * a.C * AUG_FRAME;
  if (a.n_out < need) return (int)hipErrorInvalidValue;
  if ((((uintptr_t)a.ring | (uintptr_t)a.out) & 15) || ((uintptr_t)a.slots & 3) || ((uintptr_t)a.off_out & 3))
    return (int)hipErrorInvalidValue;
  const uintptr_t r0 = (uintptr_t)a.ring, r1 = r0 + (uintptr_t)a.F * AUG_FRAME;
  const uintptr_t o0 = (uintptr_t)a.out, o1 = o0 + (uintptr_t)a.n_out;
  if (o0 < r1 && r0 < o1) return (int)hipErrorInvalidValue;
  augment_shift_kernel<<<(unsigned)(a.rows * a.C), 256, 0, st>>>(a);
  APEX_CHECK_LAUNCH();
}

// bounds violations of the ring slots seen by the debug library (count, first bad slot); the
// release library checks nothing and reports none
APEX_EXPORT int apex_augment_debug_errors(int* count, long long* first, int reset) {
  *count = 0;
  *first = 0;
#ifdef APEX_DEBUG_BOUNDS
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyFromSymbol(count, HIP_SYMBOL(aug_dbg_count), sizeof(int));
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyFromSymbol(first, HIP_SYMBOL(aug_dbg_first), sizeof(long long));
  if (e != hipSuccess) return (int)e;
  if (reset) {
    const int zc = 0;
    const long long zf = 0;
    hipMemcpyToSymbol(HIP_SYMBOL(aug_dbg_count), &zc, sizeof(zc));
    e = hipMemcpyToSymbol(HIP_SYMBOL(aug_dbg_first), &zf, sizeof(zf));
  }
  return (int)e;
#else
  (void)reset;
  return 0;
#endif
}
