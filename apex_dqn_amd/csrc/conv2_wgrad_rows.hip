// Row-resident conv2 weight gradient (split mode): dW2[co][kh][kw][ci] partial sums of
//   dY2 [N, 9, 9, 64] hi + lo  x  y1 NHWC [N, 20, 20, 64] hi + lo,  4 x 4 kernel, stride 2,
// into the same slab[split][co][kc] / bias_slab[split][co] as igemm_wgrad_kernel<1, 9, 81,
// 1, 2, 1> (csrc/igemm_wgrad.h), bit for bit: the same rows_per_split, per (split, 32-row
// half, 16 x 16 tile) one accumulator chain over the 64-row steps with the three MFMAs
// (X hi, dY lo), (X lo, dY hi), (X hi, dY hi) in that order, the half-1 sums added to the
// half-0 sums through LDS, the bias gradient from two all-ones MFMAs per step.
//
// The generic kernel stages the im2col view: every 64-row step copies two taps' X images,
// so a y1 pixel is fetched once per tap that touches it (3.24 x) and dY2 by all 8 blocks
// of a split: 249 MB per launch at 512 images, in 472 one-per-CU blocks.  Here one
// workgroup of 8 waves owns one (split, kh): all four kw taps, both halves, all 64 output
// channels; wave w owns (half = w >> 2, kw = w & 3).  Grid = 4 x nsplit (236 at 512 images).
//
// Staging, each byte once per workgroup (~139 MB per launch):
//  * dY2 rows of a step (64 x 128 B, hi + lo): buffer LDS-DMA into the swz_tr image, zeros
//    past the split end through the range check, two stages, shared by the 8 waves.
//  * y1 INPUT rows as they lie in memory: output row J = img * 9 + oh needs input row
//    2 oh + kh (20 px x 128 B, hi + lo = 5,120 B), kept in a ring of RING_D slots until no
//    later step needs it.  A slot is 40 cells of 128 B: plane (hi, lo) x pixel parity e x
//    u = pixel >> 1, at cell plane * 20 + e * 10 + (u ^ (J & 1)); five 1-KB LDS-DMA pieces.
//  * a per-workgroup table gives, per reduction row m = 9 J + ow and kw >> 1, the cell of
//    pixel 2 ow + kw (minus the e * 10 the wave adds) and the chunk swizzle; rows past the
//    split end point at a zeroed cell.
//
// Bank conflicts: a ds_read_b64_tr_b16 half-wave reads rows a .. a + 3 and a + 8 .. a + 11,
// 32 B each, of pixels 256 B apart in memory order.  With v = 9 J + u (= m + (kw >> 1) for
// the reading wave) the pixel's 128 B sit in half bit0(v) of the 256-B bank row (the cell
// parity above) and its 16-B chunk c at c ^ (f << 1), f = bit1(v) | bit3(v) << 1: the four
// rows of a quad differ in (bit0, bit1), row x + 8 differs from x in bit3, so the eight
// 32-B segments are distinct for every a (scripts/lds_conflicts_conv2_wgrad_rows.py).
//
// LDS 162,432 B (ring 24 x 5,120, zero cells 2,688, dY 2 x 16,384, table 4,096): one
// workgroup per CU.  gfx950 build: 162 VGPRs, no scratch (scripts/check_spills.py).
//
// Measured at 512 images (docs/PERF_NOTES.md): 28.8 us isolated against the generic
// kernel's 29.9 (inside the spread of either), 58.2 against 61.9 us inside the fp32 step,
// where it ends the backward; a workgroup takes 2.6-3.1 us per step whether 76 or 236 of them
// run, so the launch is bound by the workgroup's own barrier-to-barrier step, not by bytes.
#include "igemm_wgrad.h"

#define C2R_D 24                          // ring slots (input rows)
#define C2R_SLOT 5120                     // hi + lo planes of one input row
#define C2R_CELLS (C2R_D * 40)            // cell index of the zero cell (hi; lo 20 cells on)
#define C2R_LO 2560                       // lo plane of a cell
#define C2R_ZERO (C2R_D * C2R_SLOT)
#define C2R_DY (C2R_ZERO + 21 * 128)      // dY stages: hi image, lo image
#define C2R_DYSTAGE (2 * WG_IMG)
#define C2R_TBL (C2R_DY + 2 * C2R_DYSTAGE)
#define C2R_MAXROWS 1024                  // table rows (u16 entries, two per row)
#define C2R_SMEM (C2R_TBL + 2 * C2R_MAXROWS * 2)

// chunk swizzle of the pixel with v = 9 J + u
__device__ __forceinline__ int c2r_f(int v) { return ((v >> 1) & 1) | (((v >> 3) & 1) << 1); }

__global__ void __launch_bounds__(512) conv2_wgrad_rows_kernel(WgradDesc d) {
  static_assert(C2R_SMEM <= 163840, "LDS");
  static_assert((C2R_D & 1) == 0 && C2R_D >= 16, "ring: whole 1-KB pieces, two steps' rows");
  __shared__ __attribute__((aligned(256))) uint8_t smem[C2R_SMEM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = wv >> 2, kw = wv & 3;
  // XCD-contiguous order: the four kh workgroups of a split (same dY rows, overlapping
  // input rows) and neighbouring splits run on one XCD's L2
  const int wg = xcd_swizzle((int)blockIdx.x, (int)gridDim.x);
  const int kh = wg & 3, split = wg >> 2;
  const int r_begin = split * d.rows_per_split;
  const int r_end = min(d.Mred, r_begin + d.rows_per_split);
  const int nst = (r_end - r_begin + WG_ROWS - 1) / WG_ROWS;
  const int trows = nst * WG_ROWS;
  const int J0 = r_begin / 9, Jlast = (r_end - 1) / 9;   // output rows (img * 9 + oh) of the split

  // ---------------- prologue: row table + zero cells
  uint16_t* tbl = reinterpret_cast<uint16_t*>(smem + C2R_TBL);
  for (int r = tid; r < trows; r += 512) {
    const int m = r_begin + r;
    uint32_t e0 = C2R_CELLS, e1 = C2R_CELLS;
    if (m < r_end) {
      const int J = m / 9, ow = m - 9 * J;
      const int base = ((J - J0) % C2R_D) * 40;
      e0 = (uint32_t)(base + (ow ^ (J & 1))) | ((uint32_t)c2r_f(m) << 12);
      e1 = (uint32_t)(base + ((ow + 1) ^ (J & 1))) | ((uint32_t)c2r_f(m + 1) << 12);
    }
    tbl[r] = (uint16_t)e0;
    tbl[C2R_MAXROWS + r] = (uint16_t)e1;
  }
  if (tid < 8) {
    *reinterpret_cast<uint4*>(smem + C2R_ZERO + tid * 16) = make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4*>(smem + C2R_ZERO + C2R_LO + tid * 16) = make_uint4(0, 0, 0, 0);
  }

  // ---------------- staging
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  const uint8_t* xh = static_cast<const uint8_t*>(d.x);
  const uint8_t* xl = static_cast<const uint8_t*>(d.x_lo);
  // piece Q = 5 (J - J0) + k: cells 8 k .. 8 k + 7 of output row J's slot; wave Q % 8 issues it
  auto issue_piece = [&](int Q) {
    const int jr = Q / 5, k = Q - 5 * jr, J = J0 + jr;
    const int sc = 8 * k + (lane >> 3);              // slot cell 0 .. 39
    const int plane = sc >= 20 ? 1 : 0, w20 = sc - 20 * plane;
    const int e = w20 >= 10 ? 1 : 0, u = (w20 - 10 * e) ^ (J & 1);
    const int c = (lane & 7) ^ (c2r_f(9 * J + u) << 1);
    const int img = J / 9, oh = J - 9 * img;
    const size_t off = ((size_t)((img * 20 + 2 * oh + kh) * 20 + 2 * u + e) << 7) + (size_t)(c << 4);
    const uint32_t l = lds0 + (uint32_t)((jr % C2R_D) * C2R_SLOT + k * 1024);
    dma16((plane ? xl : xh) + off, __builtin_amdgcn_readfirstlane(l));
  };
  // pieces [Qa, Qb) of this wave; returns how many it issued
  auto issue_pieces = [&](int Qa, int Qb) -> int {
    int n = 0;
    for (int Q = Qa + ((wv - Qa) & 7); Q < Qb; Q += 8, ++n) issue_piece(Q);
    return n;
  };
  // dY rows of step st: thread row tid >> 3, the chunk that lands in slot tid & 7 of the swz_tr image
  const int srow = tid >> 3;
  const int sc8 = (tid & 7) ^ ((((srow >> 1) & 1) | (((srow >> 3) & 1) << 1)) << 1);
  const __amdgpu_buffer_rsrc_t dy_rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(d.dy), (short)0, r_end * 128, 0x00020000);
  const __amdgpu_buffer_rsrc_t dyl_rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(d.dy_lo), (short)0, r_end * 128, 0x00020000);
  const uint32_t dy_off = (uint32_t)((r_begin + srow) * 128 + sc8 * 16);
  auto issue_dy = [&](int st) {
    const uint32_t o = dy_off + (uint32_t)st * (WG_ROWS * 128);
    const uint32_t l = __builtin_amdgcn_readfirstlane(lds0 + C2R_DY + (uint32_t)(st & 1) * C2R_DYSTAGE + (uint32_t)wv * 1024u);
    bdma16(dy_rs, o, l);
    bdma16(dyl_rs, o, l + WG_IMG);
  };
  auto jhi = [&](int st) { return (min(r_end, r_begin + WG_ROWS * (st + 1)) - 1) / 9; };
  auto jlo = [&](int st) { return (r_begin + WG_ROWS * st) / 9; };

  // ---------------- fragments
  const int g = lane >> 4, q = (lane >> 2) & 3, pcol = lane & 3, pl = lane & 15;
  const int rA = 32 * half + 8 * g + q;
  const uint16_t* trow = tbl + (kw >> 1) * C2R_MAXROWS + rA;
  const int eoff = (kw & 1) * 1280 + 8 * pcol;
  const bool do_bias = d.bias_slab != nullptr && kh == 0 && kw == 0;
  f32x4 acc[4][4], accb[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    accb[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u));

  auto xfrag = [&](int a0, int f0, int a1, int f1, int t) -> bf16x8 {
    const lds_s16x4* pa = (const lds_s16x4*)(smem + a0 + ((t ^ f0) << 5));
    const lds_s16x4* pb = (const lds_s16x4*)(smem + a1 + ((t ^ f1) << 5));
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(const_cast<lds_s16x4*>(pa));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(const_cast<lds_s16x4*>(pb));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  uint32_t e0 = 0, e1 = 0;         // this step's table entries (rows rA, rA + 4), read a step ahead
  auto compute = [&](int st) {
    if (st == 0) e0 = trow[0], e1 = trow[4];
    const int c0 = e0 & 0xfff, c1 = e1 & 0xfff, f0 = e0 >> 12, f1 = e1 >> 12;
    // rows past the split end: the zero cell as it stands
    const int a0 = (c0 << 7) + (c0 < C2R_CELLS ? eoff : 8 * pcol);
    const int a1 = (c1 << 7) + (c1 < C2R_CELLS ? eoff : 8 * pcol);
    const uint8_t* D = smem + C2R_DY + (st & 1) * C2R_DYSTAGE;
    const uint8_t* DL = D + WG_IMG;
    if (st + 1 < nst) e0 = trow[(st + 1) * WG_ROWS], e1 = trow[(st + 1) * WG_ROWS + 4];
    bf16x8 a[4], b[4], al[4], bl[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = tr_frag8(D, half, 16 * t, lane);
      al[t] = tr_frag8(DL, half, 16 * t, lane);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      b[t] = xfrag(a0, f0, a1, f1, t);
      bl[t] = xfrag(a0 + C2R_LO, f0, a1 + C2R_LO, f1, t);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], al[i], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[j], a[i], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    if (do_bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, al[i], accb[i], 0, 0, 0);
        accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, a[i], accb[i], 0, 0, 0);
      }
    }
  };

  // ---------------- main loop.  Issue block before step s (s = 0: before the loop): (1) the
  // input rows step s still lacks, (2) its dY rows, (3) further rows as far as the ring
  // allows while the rows of step s - 1 stay.  Step s waits for (1) and (2): only this
  // wave's (3) pieces of the last block may still be in flight.
  int Qn = 0;                      // pieces issued so far (all waves)
  int ahead;                       // this wave's (3) pieces of the last block
  {
    const int q1 = 5 * (jhi(0) - J0 + 1), q3 = 5 * (min(Jlast, J0 + C2R_D - 1) - J0 + 1);
    issue_pieces(0, q1);
    issue_dy(0);
    ahead = issue_pieces(q1, q3);
    Qn = q3;
  }
  for (int st = 0; st < nst; ++st) {
    vmcnt_le(ahead);
    __syncthreads();               // step st landed; every wave is done with step st - 1
    ahead = 0;
    if (st + 1 < nst) {
      const int q1 = max(Qn, 5 * (jhi(st + 1) - J0 + 1));
      const int q3 = max(q1, 5 * (min(Jlast, jlo(st) + C2R_D - 1) - J0 + 1));
      issue_pieces(Qn, q1);
      issue_dy(st + 1);
      ahead = issue_pieces(q1, q3);
      Qn = q3;
    }
    compute(st);
  }

  // ---------------- half-1 waves hand their sums to the half-0 waves (acc then accb, lane-major)
  vmcnt_le(0);
  __syncthreads();                 // every wave is done reading the ring, no DMA in flight
  f32x4* red = reinterpret_cast<f32x4*>(smem) + kw * (20 * 64) + lane;
  if (half) {
#pragma unroll
    for (int k = 0; k < 16; ++k) red[k * 64] = acc[k >> 2][k & 3];
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(16 + i) * 64] = accb[i];
  }
  __syncthreads();
  if (half) return;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k >> 2][k & 3] += red[k * 64];
#pragma unroll
  for (int i = 0; i < 4; ++i) accb[i] += red[(16 + i) * 64];

  // ---------------- fp32 partial tile -> slab[split][co][kc], kc = (kh 4 + kw) 64 + channel
  float* slab = d.slab + (int64_t)split * 64 * 1024;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<f32x4*>(slab + (16 * i + pl) * 1024 + (kh * 4 + kw) * 64 + 16 * j + 4 * g) = acc[i][j];
  if (do_bias && g == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) d.bias_slab[(int64_t)split * 64 + 16 * i + pl] = accb[i][0];
  }
}

// 1 when the row-resident kernel covers the problem: split-mode conv2 (both lo planes), no
// fused norm partials, whole 64-row steps that fit the row table (ops/conv.py
// conv2_wgrad_rows_covers is the caller's copy of this rule)
static bool conv2_wgrad_rows_covers(const WgradDesc& d) {
  return d.mode == 1 && d.H == 20 && d.W == 20 && d.Cin == 64 && d.OH == 9 && d.OW == 9 && d.KH == 4 &&
         d.KW == 4 && d.stride == 2 && d.pad_h == 0 && d.pad_w == 0 && d.Co == 64 && d.Kc == 1024 &&
         d.ldd == 64 && d.dy_lo != nullptr && d.x_lo != nullptr && d.norm_part == nullptr &&
         d.rows_per_split > 0 && (d.rows_per_split & 63) == 0 && d.rows_per_split <= C2R_MAXROWS &&
         d.N > 0 && d.Mred == d.N * 81 && (int64_t)d.Mred * 128 < 0x7ffffff0LL;
}

APEX_EXPORT int apex_slab_reduce(const float* slab, int nsplit, int64_t n, float scale, float* out, const float* bslab,
                                 int nb, float* bout, int s2dC, int Kc, hipStream_t st);

// Same contract as apex_conv_wgrad (csrc/conv_mfma.hip) for the covered shape; anything else
// is an error (the caller picks the generic kernel).
APEX_EXPORT int apex_conv2_wgrad_rows(WgradDesc d, float* out, float* bout, int nsplit, float scale, hipStream_t st) {
  if (!conv2_wgrad_rows_covers(d)) return (int)hipErrorInvalidValue;
  if (nsplit != (d.Mred + d.rows_per_split - 1) / d.rows_per_split) return (int)hipErrorInvalidValue;
  conv2_wgrad_rows_kernel<<<4 * nsplit, 512, 0, st>>>(d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (out != nullptr)
    return apex_slab_reduce(d.slab, nsplit, (int64_t)64 * 1024, scale, out, d.bias_slab, d.bias_slab ? 64 : 0, bout, 0,
                            1024, st);
  return 0;
}
