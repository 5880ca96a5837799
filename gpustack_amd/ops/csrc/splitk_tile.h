// The split-K 128-column MFMA tile shared by the bf16 and FP8 serving GEMMs
// (skinny_gemm.hip, fp8_gemm.hip) on MI355X (gfx950).
//
//   C[M, N] = X[M, K] · W[N, K]^T, f32 accumulate, bf16 out.
//
// Measured in bytes the two GEMMs are one algorithm: an LDS row is 128 B, a
// K tile is two 64-byte half-rows, and per half-row every lane reads 16 B of
// X and of W through the same swizzle. An element policy says how many bytes
// an element has (BK = 128 / ES elements), what a lane does with its
// 16 B + 16 B, and whether the result carries row and column scales.
//
// Structure (guide §5 "minimum 2-phase" recipe, m97-style):
//  - (32*MI)x128 tile, 8 waves (2 row halves x 4 column quarters), per-wave
//    output (16*MI)x32; double-buffered LDS (96 KiB at MI=8)
//  - global->LDS staging via __builtin_amdgcn_global_load_lds width 16
//    with the XOR swizzle applied on the PRE-SWIZZLED GLOBAL SOURCE (guide
//    m173: gload_lds writes linearly, so the source permutation carries the
//    swizzle; ds_read applies the same XOR)
//  - SPLITK partials in f32 workspace + a reduce/convert kernel
//    (two-pass: deterministic, no atomics)
#pragma once

#include "common.h"

namespace splitk {

constexpr int BN = 128;
constexpr int ROW_BYTES = 128;
constexpr int WAVES = 8;
constexpr int THREADS = WAVES * WAVE_SIZE;

typedef __attribute__((ext_vector_type(2))) long i64x2;   // a 16-B fragment
typedef __attribute__((ext_vector_type(8))) short s16x8;

// LDS tiles are rows x 128 bytes; XOR-swizzle byte offsets within each row
// to kill the 16-way ds_read_b128 bank conflict.
DEVICE_INLINE int swz_col(int row, int colbyte) {
  return colbyte ^ ((row & 7) << 4);
}
DEVICE_INLINE int swz(int row, int colbyte) {
  return row * ROW_BYTES + swz_col(row, colbyte);
}

struct Bf16 {
  static constexpr int ES = 2;
  static constexpr bool SCALED = false;
  static constexpr bool COLS_OUTER = false;
  DEVICE_INLINE static f32x4 mma(i64x2 a, i64x2 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        __builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), c, 0, 0, 0);
  }
};

// OCP e4m3 codes with one f32 scale per X row and per W row. The fp8
// instruction takes 8 B of A and B per lane. Read as ds_read_b64 through the
// swizzle, the 32 lanes of a half-wave would touch 16 rows x 2 eight-byte
// halves; rows r and r+8 have equal (row&7) and equal parity, i.e. the same
// 16-B slot of the 256-B bank row, so that read is 2-way conflicted (the
// swizzle only separates 8 rows, which is all a 16-lane ds_read_b128 group
// needs). Instead each lane keeps the bf16 kernel's conflict-free
// ds_read_b128 and feeds its low and high 8 B to two consecutive MFMAs. That
// permutes k inside a 64-byte half-row (lane group g supplies bytes
// 16g..16g+7 to the first MFMA and 16g+8..16g+15 to the second), identically
// for A and B, so the dot product is unchanged and the kernel issues half
// the LDS reads.
struct Fp8 {
  static constexpr int ES = 1;
  static constexpr bool SCALED = true;
  static constexpr bool COLS_OUTER = true;
  DEVICE_INLINE static f32x4 mma(i64x2 a, i64x2 b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[0], b[0], c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[1], b[1], c, 0, 0, 0);
  }
};

// Stage ROWS x 128 B of a row-major [nrows, K] matrix of ES-byte elements,
// from (row0, kbase), into linear LDS at `lds`. Each thread owns fixed linear
// 16-B chunks; linear LDS byte L of a chunk maps to logical (row = L/128,
// colbyte = (L%128) ^ swz(row)) and the global source reads that element.
// CLAMP reads row nrows-1 for rows past the end (masked at write); without
// it the caller guarantees the rows are in range.
template <int ROWS, int ES, bool CLAMP>
DEVICE_INLINE void stage_rows(char* lds, const void* g, int row0, int nrows,
                              int K, long kbase, int t) {
  constexpr int CHUNKS = ROWS * ROW_BYTES / 16 / THREADS;
  static_assert(CHUNKS >= 1, "tile must give every thread a chunk");
#pragma unroll
  for (int r = 0; r < CHUNKS; ++r) {
    const int L = (t + r * THREADS) * 16;
    const int row = L / ROW_BYTES;
    int grow = row0 + row;
    if (CLAMP && grow >= nrows) grow = nrows - 1;
    // row and K offsets are scaled separately: ((grow*K + kbase) * ES) cost
    // the bf16 kernel 12 more VGPRs
    const char* src = reinterpret_cast<const char*>(g) +
                      (long)grow * K * ES + kbase * ES +
                      swz_col(row, L % ROW_BYTES);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(lds + L), 16, 0, 0);
  }
}

DEVICE_INLINE i64x2 read_frag(const char* lds, int row, int colbyte) {
  return *reinterpret_cast<const i64x2*>(lds + swz(row, colbyte));
}

// Which split, rows, columns and K range a block owns. kchunk = K/splitk is
// a multiple of BK (host-checked).
struct Tile { int split, m0, n0, k0, nk; };

template <int BM, int BN_, int BK>
DEVICE_INLINE Tile tile_decode(int M, int K, int splitk) {
  const int mt = (M + BM - 1) / BM;
  int tid = blockIdx.x;
  Tile tl;
  tl.split = tid % splitk;
  tid /= splitk;
  tl.m0 = (tid % mt) * BM;
  tl.n0 = (tid / mt) * BN_;
  const int kchunk = K / splitk;
  tl.k0 = tl.split * kchunk;
  tl.nk = kchunk / BK;
  return tl;
}

// Store a wave's MI x 2 accumulator fragments whose top-left element is
// (row0, col0): D row = (l>>4)*4 + r, col = l&15 per 16x16 fragment. Partials
// go to the f32 workspace unscaled. The direct path rounds to bf16 once; when
// SCALED the scales multiply the f32 sum before that rounding (with split-K
// the reduce kernel does that on the final sum instead). COLS_OUTER walks
// the fragments column-outer (one column scale per pass) instead of
// row-outer. The order does not change results, but it moves the time of
// large partial writes by several percent either way
// (profiles/splitk_tile.md), so each kernel keeps the order it was measured
// with.
template <bool SCALED, bool WRITE_PARTIAL, bool COLS_OUTER, int MI>
DEVICE_INLINE void store_frags(void* out, const f32x4 (&acc)[MI][2],
                               const float* xs, const float* ws, int row0,
                               int col0, int split, int M, int N, int lane) {
  const int lc = lane & 15;
  const int lg = lane >> 4;
  float wsc[2] = {1.f, 1.f};
  if constexpr (SCALED && !WRITE_PARTIAL) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) wsc[ni] = ws[col0 + ni * 16 + lc];
  }
#pragma unroll
  for (int f = 0; f < MI * 2; ++f) {
    const int mi = COLS_OUTER ? f % MI : f / 2;
    const int ni = COLS_OUTER ? f / MI : f % 2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int grow = row0 + mi * 16 + lg * 4 + r;
      const int gcol = col0 + ni * 16 + lc;
      if (grow >= M) continue;
      if constexpr (WRITE_PARTIAL) {
        reinterpret_cast<float*>(out)[((long)split * M + grow) * N + gcol] =
            acc[mi][ni][r];
      } else if constexpr (SCALED) {
        reinterpret_cast<unsigned short*>(out)[(long)grow * N + gcol] =
            f2bf(acc[mi][ni][r] * xs[grow] * wsc[ni]);
      } else {
        reinterpret_cast<unsigned short*>(out)[(long)grow * N + gcol] =
            f2bf(acc[mi][ni][r]);
      }
    }
  }
}

// One block's (32*MI) x 128 tile of one K split. out is bf16 [M,N], or the
// f32 [S,M,N] workspace when WRITE_PARTIAL; xs [M] and ws [N] are read only
// when Elem::SCALED. W rows are not clamped (N % 128 == 0, host-checked): a
// clamp there adds instructions inside the K loop.
template <class Elem, int MI, bool WRITE_PARTIAL>
DEVICE_INLINE void tile_body(void* out, const void* x, const float* xs,
                             const void* w, const float* ws, int M, int N,
                             int K, int splitk) {
  constexpr int ES = Elem::ES;
  constexpr int BM = 32 * MI;
  constexpr int BK = ROW_BYTES / ES;
  const Tile tl = tile_decode<BM, BN, BK>(M, K, splitk);

  __shared__ __attribute__((aligned(16))) char Xl[2][BM * ROW_BYTES];
  __shared__ __attribute__((aligned(16))) char Wl[2][BN * ROW_BYTES];

  const int t = threadIdx.x;
  const int lane = t & (WAVE_SIZE - 1);
  const int wid = t / WAVE_SIZE;
  const int wm = wid >> 2;               // 0..1  (row half)
  const int wn = wid & 3;                // 0..3  (col quarter)
  const int lc = lane & 15;
  const int lg = lane >> 4;

  auto stage = [&](int buf, int kb) {
    const long kbase = tl.k0 + (long)kb * BK;
    stage_rows<BM, ES, true>(Xl[buf], x, tl.m0, M, K, kbase, t);
    stage_rows<BN, ES, false>(Wl[buf], w, tl.n0, N, K, kbase, t);
  };

  f32x4 acc[MI][2];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  int buf = 0;
  for (int kb = 0; kb < tl.nk; ++kb) {
    if (kb + 1 < tl.nk) stage(buf ^ 1, kb + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {          // 64-byte half-row
      const int colbyte = h * 64 + lg * 16;
      i64x2 bfrag[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)       // W row (output col)
        bfrag[ni] = read_frag(Wl[buf], wn * 32 + ni * 16 + lc, colbyte);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {    // X row (output row)
        const i64x2 a =
            read_frag(Xl[buf], wm * (16 * MI) + mi * 16 + lc, colbyte);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = Elem::mma(a, bfrag[ni], acc[mi][ni]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    buf ^= 1;
  }

  store_frags<Elem::SCALED, WRITE_PARTIAL, Elem::COLS_OUTER>(
      out, acc, xs, ws, tl.m0 + wm * (16 * MI), tl.n0 + wn * 32, tl.split, M,
      N, lane);
}

// partial[S, M, N] f32 -> out[M, N] bf16; fixed summation order, no atomics.
// When SCALED the final sum is multiplied by xs[row] * ws[col] once.
template <bool SCALED>
__global__ void splitk_reduce_kernel(unsigned short* __restrict__ out,
                                     const float* __restrict__ partial,
                                     const float* __restrict__ xs,
                                     const float* __restrict__ ws, long MN,
                                     int N, int splitk) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < MN;
       i += (long)gridDim.x * blockDim.x) {
    float a = 0.f;
    for (int s = 0; s < splitk; ++s) a += partial[s * MN + i];
    if constexpr (SCALED) a = a * xs[i / N] * ws[i % N];
    out[i] = f2bf(a);
  }
}

// Every tile kernel takes these operands; xs and ws are null without scales.
using TileKernel = void (*)(void*, const void*, const float*, const void*,
                            const float*, int, int, int, int);

// splitk > 1: the partial kernel fills workspace [S,M,N], then the reduce
// kernel writes out; otherwise the direct kernel writes out.
template <int BM, int BN_, bool SCALED>
inline void launch(TileKernel partial, TileKernel direct, void* out,
                   const void* x, const float* xs, const void* w,
                   const float* ws, void* workspace, int M, int N, int K,
                   int splitk, hipStream_t s) {
  const int mt = (M + BM - 1) / BM;
  const int nt = N / BN_;
  const dim3 grid(mt * nt * splitk);
  const dim3 block(THREADS);
  if (splitk > 1) {
    hipLaunchKernelGGL(partial, grid, block, 0, s, workspace, x, xs, w, ws, M,
                       N, K, splitk);
    const long MN = (long)M * N;
    int rgrid = (int)((MN + 255) / 256);
    if (rgrid > 2048) rgrid = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel<SCALED>, dim3(rgrid), dim3(256), 0,
                       s, (unsigned short*)out, (const float*)workspace, xs,
                       ws, MN, N, splitk);
  } else {
    hipLaunchKernelGGL(direct, grid, block, 0, s, out, x, xs, w, ws, M, N, K,
                       splitk);
  }
}

}  // namespace splitk
