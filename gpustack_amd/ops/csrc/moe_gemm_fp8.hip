// Grouped MoE expert GEMMs on FP8 expert banks for MI355X (gfx950): the
// W8A8 siblings of moe_gemm.hip for quantize_runtime="fp8_moe" (OCP e4m3
// codes, one f32 scale per token row and per expert output row).
//
//   moe_gate_up_silu_fp8: act[j, :] = bf16( silu(g) * u )
//       g = (xq[tok_j] . Wgq[e_j]^T) * xs[tok_j] * wsg[e_j]
//       u likewise with the up half of the bank
//   moe_down_scale_fp8:   contrib[order[j], :] =
//       bf16( (aq[j] . Wdq[e_j]^T) * as[j] * wsd[e_j] * w_j )
//
// Same contract as the bf16 pair: fixed E x N/64 grids independent of the
// routing outcome, workgroups of empty experts exit at once, no host sync,
// no atomics, the s_tok / order / offs / counts lists of moe_align.
//
// The design follows the one-byte stream rather than the bf16 kernel:
//  - a lane's 16 B weight load and its 16 B LDS A read each feed TWO
//    v_mfma_f32_16x16x32_fp8_fp8, one from the low and one from the high
//    8 B (the pairing of splitk_tile.h's Fp8 element), so one load step
//    covers 64 K codes. Lane group g supplies codes 16g..16g+7 to the first
//    MFMA and 16g+8..16g+15 to the second, identically for A and B: a
//    permutation of k inside the 64-code step, which leaves every dot
//    product unchanged (fp8_mfma_probe pins the per-instruction lane map);
//  - the K chunk staged in LDS is 1024 codes — the bf16 kernel's 512
//    elements in bytes — so the fully unrolled chunk keeps the same number
//    of 16 B weight loads in flight per wave (32 gate+up, 16 down) over
//    twice the K;
//  - a weight pass serves up to 32 rows: two 16-row m-tiles of gathered
//    codes are staged per chunk and every loaded weight fragment is issued
//    against both, so an expert holding 17..32 rows streams its panel once.
//    The second tile's MFMAs sit behind a wave-uniform branch;
//  - scales touch only the f32 accumulators in the epilogue, in the order
//    of torch_ref.fp8_gemm (row scale, then column scale), followed by one
//    bf16 rounding.
#include "common.h"

namespace {

constexpr int M8_BN = 64;         // N columns per workgroup (16 per wave)
constexpr int M8_KC = 1024;       // K codes per LDS chunk
constexpr int M8_KS = 64;         // K codes per load step (2 MFMAs)
constexpr int M8_ROWS = 32;       // rows per weight pass (two m-tiles)
constexpr int M8_THREADS = 256;   // 4 waves
// LDS row stride in bytes. A-fragment reads are ds_read_b128: lane (lc, lg)
// reads 16 B at row lc, byte kk + 16*lg. The 64 banks x 4 B make a 256-B
// bank row of sixteen 16-B slots, and a 16-lane group is served together.
// With an unpadded 1024-B row all 16 rows of a group would start in slot 0
// (16-way conflict). 16 B of padding shifts row r by r slots, so the group
// with a given lg touches slots (lc + lg + kk/16) mod 16, lc = 0..15: all
// sixteen slots once, every bank once. The staging writes put consecutive
// lanes on consecutive 16-B units of one row and are conflict free too.
constexpr int M8_LDS_ROW = M8_KC + 16;

typedef __attribute__((ext_vector_type(2))) long m8_i64x2;  // 16 B of codes

// both halves of a 16-B A/B pair: 64 K codes
DEVICE_INLINE f32x4 m8_mfma2(m8_i64x2 a, m8_i64x2 b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[0], b[0], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[1], b[1], c, 0, 0, 0);
}

// Stage rows [rows16][kc] of e4m3 codes into LDS, rows16 = 16 or 32: only
// the m-tiles that will be read. Rows past nrows are zero (their products
// land in accumulator rows the epilogue skips). GATHER takes row r from
// src[tok[r]], otherwise from src[base_row + r].
template <bool GATHER>
DEVICE_INLINE void m8_stage_rows(unsigned char* lds, const unsigned char* src,
                                 long src_stride, const int* tok, int base_row,
                                 int nrows, int k0, int kc, int tid) {
  const int per_row = kc / 16;               // 16-B units per row
  const int units = (nrows > 16 ? 32 : 16) * per_row;
  for (int u = tid; u < units; u += M8_THREADS) {
    const int row = u / per_row;
    const int kk = (u % per_row) * 16;
    m8_i64x2 val = {0, 0};
    if (row < nrows) {
      const long r = GATHER ? (long)tok[row] : (long)(base_row + row);
      val = *reinterpret_cast<const m8_i64x2*>(src + r * src_stride + k0 + kk);
    }
    *reinterpret_cast<m8_i64x2*>(lds + row * M8_LDS_ROW + kk) = val;
  }
}

// One K chunk of NB weight panels (2: gate and up, 1: down) against one or
// two staged m-tiles. acc[b][t] is panel b, m-tile t. wp[b] points at this
// lane's weight row at the chunk's first code plus the lane group's 16 B.
// The kernels are weight-stream bound, so a full chunk first issues all of
// its 16*NB weight loads (constexpr trip counts: the buffer is fully
// unrolled into registers — see moe_gemm.hip, runtime-indexed register
// buffers measured 10x slower) and only then walks the MFMAs, which wait on
// the loads in issue order. The runtime loop serves the tail chunk.
template <int NB, bool TWO>
DEVICE_INLINE void m8_chunk(f32x4 (&acc)[NB][2], const unsigned char* al,
                            const unsigned char* const (&wp)[NB], int kc) {
  auto mma = [&](int kk, const m8_i64x2 (&b)[NB]) {
    const m8_i64x2 a0 = *reinterpret_cast<const m8_i64x2*>(al + kk);
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i][0] = m8_mfma2(a0, b[i], acc[i][0]);
    if constexpr (TWO) {
      const m8_i64x2 a1 =
          *reinterpret_cast<const m8_i64x2*>(al + 16 * M8_LDS_ROW + kk);
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[i][1] = m8_mfma2(a1, b[i], acc[i][1]);
    }
  };
  if (kc == M8_KC) {
    constexpr int STEPS = M8_KC / M8_KS;
    m8_i64x2 b[STEPS][NB];
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int i = 0; i < NB; ++i)
        b[s][i] = *reinterpret_cast<const m8_i64x2*>(wp[i] + s * M8_KS);
    // left alone, the scheduler sinks the loads back between the MFMAs to
    // save registers and the wave has 2-4 loads in flight instead of 16*NB
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) mma(s * M8_KS, b[s]);
  } else {
    for (int kk = 0; kk < kc; kk += M8_KS) {
      m8_i64x2 b[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i)
        b[i] = *reinterpret_cast<const m8_i64x2*>(wp[i] + kk);
      mma(kk, b);
    }
  }
}

__global__ __launch_bounds__(M8_THREADS) void moe_gate_up_silu_fp8_kernel(
    unsigned short* __restrict__ act,       // [TK, I] bf16 (sorted rows)
    const unsigned char* __restrict__ xq,   // [T, H] e4m3
    const float* __restrict__ xs,           // [T]
    const unsigned char* __restrict__ wq,   // [E, 2I, H] e4m3 (gate then up)
    const float* __restrict__ ws,           // [E, 2I]
    const int* __restrict__ s_tok,          // [TK] token index per sorted row
    const int* __restrict__ offs,           // [E]
    const int* __restrict__ counts,         // [E]
    int H, int I) {
  const int nnt = I / M8_BN;
  const int e = blockIdx.x / nnt;
  const int nt = blockIdx.x % nnt;
  const int cnt = counts[e];
  if (cnt == 0) return;
  const int base = offs[e];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int lc = lane & 15;
  const int lg = lane >> 4;

  __shared__ __attribute__((aligned(16))) unsigned char Xl[M8_ROWS * M8_LDS_ROW];

  // this lane's output column; also its weight row inside the wave's panel
  const int col = nt * M8_BN + wave * 16 + lc;
  const unsigned char* wg_row = wq + ((long)e * 2 * I + col) * H + lg * 16;
  const unsigned char* wu_row = wg_row + (long)I * H;
  const unsigned char* al = Xl + lc * M8_LDS_ROW + lg * 16;
  // column scales depend on the lane only: one pair of loads per block
  const float wsg = ws[(long)e * 2 * I + col];
  const float wsu = ws[(long)e * 2 * I + I + col];

  for (int m0 = 0; m0 < cnt; m0 += M8_ROWS) {
    const int nrows = min(M8_ROWS, cnt - m0);
    const int* tok = s_tok + base + m0;
    f32x4 acc[2][2];                         // [gate, up][m-tile]
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < H; k0 += M8_KC) {
      const int kc = min(M8_KC, H - k0);
      __syncthreads();
      m8_stage_rows<true>(Xl, xq, H, tok, 0, nrows, k0, kc, tid);
      __syncthreads();
      const unsigned char* const wp[2] = {wg_row + k0, wu_row + k0};
      if (nrows > 16) m8_chunk<2, true>(acc, al, wp, kc);
      else m8_chunk<2, false>(acc, al, wp, kc);
    }
    // D[row = lg*4 + r][col = lc] per m-tile: scale, activate, round once
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = t * 16 + lg * 4 + r;
        if (row >= nrows) continue;
        const float rs = xs[tok[row]];
        const float g = acc[0][t][r] * rs * wsg;
        const float u = acc[1][t][r] * rs * wsu;
        act[(long)(base + m0 + row) * I + col] =
            f2bf(g / (1.f + __expf(-g)) * u);
      }
    }
  }
}

__global__ __launch_bounds__(M8_THREADS) void moe_down_scale_fp8_kernel(
    unsigned short* __restrict__ contrib,   // [TK, H] bf16 (original order)
    const unsigned char* __restrict__ aq,   // [TK, I] e4m3 (sorted rows)
    const float* __restrict__ as,           // [TK]
    const unsigned char* __restrict__ wq,   // [E, H, I] e4m3
    const float* __restrict__ ws,           // [E, H]
    const int* __restrict__ offs,           // [E]
    const int* __restrict__ counts,         // [E]
    const int* __restrict__ order,          // [TK] sorted -> original index
    const float* __restrict__ flat_w,       // [TK] routing weight (original)
    int H, int I) {
  const int nnt = H / M8_BN;
  const int e = blockIdx.x / nnt;
  const int nt = blockIdx.x % nnt;
  const int cnt = counts[e];
  if (cnt == 0) return;
  const int base = offs[e];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int lc = lane & 15;
  const int lg = lane >> 4;

  __shared__ __attribute__((aligned(16))) unsigned char Al[M8_ROWS * M8_LDS_ROW];

  const int col = nt * M8_BN + wave * 16 + lc;
  const unsigned char* wd_row = wq + ((long)e * H + col) * I + lg * 16;
  const unsigned char* al = Al + lc * M8_LDS_ROW + lg * 16;
  const float wsd = ws[(long)e * H + col];

  for (int m0 = 0; m0 < cnt; m0 += M8_ROWS) {
    const int nrows = min(M8_ROWS, cnt - m0);
    f32x4 acc[1][2];
    acc[0][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[0][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < I; k0 += M8_KC) {
      const int kc = min(M8_KC, I - k0);
      __syncthreads();
      // act rows are consecutive in sorted space
      m8_stage_rows<false>(Al, aq, I, nullptr, base + m0, nrows, k0, kc, tid);
      __syncthreads();
      const unsigned char* const wp[1] = {wd_row + k0};
      if (nrows > 16) m8_chunk<1, true>(acc, al, wp, kc);
      else m8_chunk<1, false>(acc, al, wp, kc);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = t * 16 + lg * 4 + r;
        if (row >= nrows) continue;
        const int j = base + m0 + row;
        const int oj = order[j];
        contrib[(long)oj * H + col] =
            f2bf(acc[0][t][r] * as[j] * wsd * flat_w[oj]);
      }
    }
  }
}

// both GEMMs need N % 64 and K % 64; H and I each play both roles
inline bool m8_dims_ok(int E, int H, int I) {
  return E >= 1 && H >= 128 && I >= 128 && H % 128 == 0 && I % 128 == 0 &&
         H % M8_KS == 0 && I % M8_KS == 0;
}

}  // namespace

void moe_gate_up_silu_fp8_launch(void* act, const void* xq, const float* xs,
                                 const void* wq, const float* ws,
                                 const int* s_tok, const int* offs,
                                 const int* counts, int E, int H, int I,
                                 int* err_unsupported, hipStream_t s) {
  *err_unsupported = !m8_dims_ok(E, H, I);
  if (*err_unsupported) return;
  hipLaunchKernelGGL(moe_gate_up_silu_fp8_kernel, dim3(E * (I / M8_BN)),
                     dim3(M8_THREADS), 0, s, (unsigned short*)act,
                     (const unsigned char*)xq, xs, (const unsigned char*)wq,
                     ws, s_tok, offs, counts, H, I);
}

void moe_down_scale_fp8_launch(void* contrib, const void* aq, const float* as,
                               const void* wq, const float* ws,
                               const int* offs, const int* counts,
                               const int* order, const float* flat_w, int E,
                               int H, int I, int* err_unsupported,
                               hipStream_t s) {
  *err_unsupported = !m8_dims_ok(E, H, I);
  if (*err_unsupported) return;
  hipLaunchKernelGGL(moe_down_scale_fp8_kernel, dim3(E * (H / M8_BN)),
                     dim3(M8_THREADS), 0, s, (unsigned short*)contrib,
                     (const unsigned char*)aq, as, (const unsigned char*)wq,
                     ws, offs, counts, order, flat_w, H, I);
}
