// Split-K skinny GEMM for decode-shaped projections on MI355X (gfx950).
//
// C[M, N] = X[M, K] · W[N, K]^T, bf16 in / bf16 out, f32 accumulate.
// Decode GEMMs (M = batch rows 256-1024, N = 4-28k) leave hipBLASLt ~2.6x
// off the weight-stream roofline at M<=256 because (N/BN)x(M/BM) tiles
// cannot fill 256 CUs; this kernel splits K so the grid covers the chip
// and streams W exactly once.
//
// v1 is the shared split-K tile of splitk_tile.h with the bf16 element:
// 256x128 tile, BK=64, mfma_f32_16x16x32_bf16, per-wave output 128x32
// (16 fragments).
#include "splitk_tile.h"

namespace {

using namespace splitk;

constexpr int BM = 256;
constexpr int BK = ROW_BYTES / Bf16::ES;

template <bool WRITE_PARTIAL>
__global__ __launch_bounds__(THREADS) void skinny_gemm_kernel(
    void* __restrict__ out,            // bf16 [M,N] or f32 [S,M,N]
    const void* __restrict__ x,        // [M, K] bf16
    const float* __restrict__ xs,      // unused: bf16 carries no scales
    const void* __restrict__ w,        // [N, K] bf16
    const float* __restrict__ ws, int M, int N, int K, int splitk) {
  tile_body<Bf16, BM / 32, WRITE_PARTIAL>(out, x, xs, w, ws, M, N, K, splitk);
}

}  // namespace

// ---------------------------------------------------------------------------
// v2: 8-phase counted-vmcnt schedule (guide §5 256^2 template, re-derived).
//
// 256x256 tile, BK=64, 8 waves each owning a 256x32 C strip. Per K-tile:
// 4 phases; phase q computes C rows [64q, 64q+64) (16 MFMA) while staging
// one half-tile of the NEXT K-tile (order B0,B1,A0,A1). Counted waits —
// vmcnt(4) after phase 1, vmcnt(2) after phase 3 — keep 2-4 staging loads
// in flight across barriers (never drained to 0 in the loop); safety is by
// construction: every wave issues the same load sequence, so its own
// vmcnt(N) + the phase barrier guarantees the half-tiles older than N are
// visible to ALL waves before any wave reads them.
// ---------------------------------------------------------------------------
namespace {

constexpr int V2_BM = 256;
constexpr int V2_BN = 256;

template <bool WRITE_PARTIAL>
__global__ __launch_bounds__(THREADS) void skinny_gemm_v2_kernel(
    void* __restrict__ out,
    const void* __restrict__ x,        // [M, K] bf16
    const float* __restrict__ xs,      // unused: bf16 carries no scales
    const void* __restrict__ w,        // [N, K] bf16
    const float* __restrict__ ws, int M, int N, int K, int splitk) {
  const Tile tl = tile_decode<V2_BM, V2_BN, BK>(M, K, splitk);

  __shared__ __attribute__((aligned(16))) char Xl[2][V2_BM * ROW_BYTES];
  __shared__ __attribute__((aligned(16))) char Wl[2][V2_BN * ROW_BYTES];

  const int t = threadIdx.x;
  const int lane = t & (WAVE_SIZE - 1);
  const int wid = t / WAVE_SIZE;          // wave's 32-col C strip
  const int lc = lane & 15;
  const int lg = lane >> 4;

  // one half-tile (128 rows x 64 cols = 16 KiB) per phase; stage order
  // within a tile's 4 phases: B0, B1, A0, A1. A half lands at its first
  // row's place in the tile (row0 % 256). W rows are in range
  // (N % 256 == 0, host-checked).
  auto stage_phase = [&](int buf, int kb, int q) {
    const long kbase = tl.k0 + (long)kb * BK;
    const int row0 = (q < 2 ? tl.n0 : tl.m0) + (q & 1) * 128;
    if (q < 2)
      stage_rows<128, Bf16::ES, false>(
          Wl[buf] + (row0 % V2_BN) * ROW_BYTES, w, row0, N, K, kbase, t);
    else
      stage_rows<128, Bf16::ES, true>(
          Xl[buf] + (row0 % V2_BM) * ROW_BYTES, x, row0, M, K, kbase, t);
  };

  f32x4 acc[16][2];
#pragma unroll
  for (int mi = 0; mi < 16; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: full tile 0
#pragma unroll
  for (int q = 0; q < 4; ++q) stage_phase(0, 0, q);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  int buf = 0;
  for (int kb = 0; kb < tl.nk; ++kb) {
    const bool more = kb + 1 < tl.nk;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (more) stage_phase(buf ^ 1, kb + 1, q);
      // B-frags: wave's 32-col strip (W rows wid*32 + ni*16 + lc)
      i64x2 bfrag[2][2];  // [ni][kk]
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          bfrag[ni][kk] = read_frag(Wl[buf], wid * 32 + ni * 16 + lc,
                                    kk * 64 + lg * 16);
      // A-frags: C rows [64q, 64q+64)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int arow = q * 64 + mi * 16 + lc;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const i64x2 a = read_frag(Xl[buf], arow, kk * 64 + lg * 16);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[q * 4 + mi][ni] =
                Bf16::mma(a, bfrag[ni][kk], acc[q * 4 + mi][ni]);
          __builtin_amdgcn_s_setprio(0);
        }
      }
      if (more) {
        if (q == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (q == 3) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else if (q == 3) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
    }
    buf ^= 1;
  }

  store_frags<false, WRITE_PARTIAL, false>(out, acc, xs, ws, tl.m0,
                                           tl.n0 + wid * 32, tl.split, M, N,
                                           lane);
}

}  // namespace

void skinny_gemm_v2_launch(void* out, const void* x, const void* w,
                           void* workspace, int M, int N, int K, int splitk,
                           hipStream_t s) {
  launch<V2_BM, V2_BN, false>(skinny_gemm_v2_kernel<true>,
                              skinny_gemm_v2_kernel<false>, out, x, nullptr,
                              w, nullptr, workspace, M, N, K, splitk, s);
}

void skinny_gemm_launch(void* out, const void* x, const void* w,
                        void* workspace, int M, int N, int K, int splitk,
                        hipStream_t s) {
  launch<BM, BN, false>(skinny_gemm_kernel<true>, skinny_gemm_kernel<false>,
                        out, x, nullptr, w, nullptr, workspace, M, N, K,
                        splitk, s);
}
