// Grouped multi-LoRA shrink/expand for MI355X (gfx950): one launch pair per
// call site (qkv, o, gate_up, down), whatever the number of adapters and
// projections in the batch.
//
//   out[row, j] += sum_r h[row, p(j)*R + r] * B_site[slot(row), j, r]
//   h[row, :]    = x[row, :] @ A_site[slot(row)]^T            ([P*R] wide)
//
// A_site [S, P*R, K] stacks the site's P projections along the rank axis,
// B_site [S, N, R] carries alpha/r; ranks below R and projections an
// adapter lacks are zero rows. The host sorts the adapter rows by slot once
// per batch into row_idx[Tl] and cuts them into tiles (slot, first,
// count <= 16): a tile never spans two slots and every adapter row is in
// exactly one tile, so the read-modify-write of `out` has no race and rows
// without an adapter are never touched. Fixed grids, no atomics, no syncs.
//
// lora_shrink_kernel<R_TOTAL>: grid (tiles, ksplit), 4 waves. N = P*R is
//   tiny and K long, so the work is cut along K only: a block owns a
//   balanced run of 32-wide K steps, its waves disjoint sub-runs. Each wave
//   streams its x rows (gathered through row_idx) and A rows straight from
//   HBM as 16 B MFMA fragments — nothing is shared between waves, so no LDS
//   staging — and keeps all R_TOTAL/16 accumulators. The four waves merge
//   through LDS in a fixed order and write one f32 partial
//   ws[kz, first + row, :] per block.
// lora_expand_add_kernel<R>: grid (tiles, N/256), 4 waves. Every lane sums
//   the ksplit partials of its h fragment in f32 as it loads them (the fused
//   split-K reduce), rounds to bf16 once and keeps the P fragments in
//   registers for the whole chunk. h rides the MFMA's column operand and
//   the B rows its row operand, so a lane ends up with four adjacent output
//   columns of ONE token row: the f32 add into `out` is a single 8 B load
//   and store per lane, rounded to bf16 once.
#include "common.h"

namespace {

constexpr int LORA_THREADS = 256;  // 4 waves
constexpr int LORA_WAVES = LORA_THREADS / WAVE_SIZE;
constexpr int LORA_NCHUNK = 256;   // expand: output columns per block

typedef __attribute__((ext_vector_type(8))) short l_s16x8;

DEVICE_INLINE f32x4 lora_mfma(u16x8 a, u16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(l_s16x8, a), __builtin_bit_cast(l_s16x8, b), c, 0, 0, 0);
}

// balanced cut of n items into `parts` runs: run p is [cut(p), cut(p+1))
DEVICE_INLINE int lora_cut(int n, int parts, int p) {
  return (int)((long)n * p / parts);
}

struct LoraTile {
  int slot, first, count;
};

// A tile the tables cannot back (slot past the bank, rows past row_idx) is
// dropped whole rather than read out of bounds.
DEVICE_INLINE LoraTile lora_tile(const int* tiles, int t, int S, int Tl) {
  LoraTile r{tiles[3 * t], tiles[3 * t + 1], tiles[3 * t + 2]};
  if (r.slot <= 0 || r.slot >= S || r.first < 0 || r.count > 16 ||
      r.first + r.count > Tl)
    r.count = 0;
  return r;
}

template <int R_TOTAL>
__global__ __launch_bounds__(LORA_THREADS) void lora_shrink_kernel(
    float* __restrict__ ws,                 // [ksplit, Tl, R_TOTAL] f32
    const unsigned short* __restrict__ x,   // [T, K] bf16
    const unsigned short* __restrict__ A,   // [S, R_TOTAL, K] bf16
    const int* __restrict__ row_idx,        // [Tl] rows with a slot, by slot
    const int* __restrict__ tiles,          // [ntiles, 3] slot, first, count
    int K, int T, int Tl, int S) {
  constexpr int NT = R_TOTAL / 16;
  constexpr int LDW = R_TOTAL + 4;  // row pad: the four row groups of a
                                    // wave's store land 16 banks apart
  constexpr int UNROLL = NT >= 8 ? 1 : (NT >= 3 ? 2 : 4);
  __shared__ float part[LORA_WAVES * 16 * LDW];

  const LoraTile tl = lora_tile(tiles, blockIdx.x, S, Tl);
  if (tl.count <= 0) return;
  const int kz = blockIdx.y, ksplit = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int lc = lane & 15;
  const int lg = lane >> 4;

  // this block's run of 32-wide K steps, then this wave's share of it
  const int steps = K / 32;
  const int b0 = lora_cut(steps, ksplit, kz);
  const int nb = lora_cut(steps, ksplit, kz + 1) - b0;
  const int s0 = b0 + lora_cut(nb, LORA_WAVES, wave);
  const int s1 = b0 + lora_cut(nb, LORA_WAVES, wave + 1);

  int row = lc < tl.count ? row_idx[tl.first + lc] : -1;
  if (row >= T) row = -1;
  const bool live = row >= 0;  // rows past the count load as zero
  const unsigned short* xrow = x + (long)(live ? row : 0) * K + lg * 8;
  const unsigned short* arow = A + ((long)tl.slot * R_TOTAL + lc) * K + lg * 8;

  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto step = [&](int s) {
    const int k0 = s * 32;
    // dead lanes read row 0 (always there) and drop it: no branch in the loop
    u16x8 xv = *reinterpret_cast<const u16x8*>(xrow + k0);
    if (!live) xv = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const u16x8 av =
          *reinterpret_cast<const u16x8*>(arow + (long)n * 16 * K + k0);
      acc[n] = lora_mfma(xv, av, acc[n]);  // D[row lg*4+r][rank n*16+lc]
    }
  };
  // UNROLL steps per trip keep enough 16 B loads in flight at small NT
  int s = s0;
  for (; s + UNROLL <= s1; s += UNROLL) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) step(s + u);
  }
  for (; s < s1; ++s) step(s);

#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      part[(wave * 16 + lg * 4 + r) * LDW + n * 16 + lc] = acc[n][r];
  __syncthreads();
  float* dst = ws + ((long)kz * Tl + tl.first) * R_TOTAL;
  for (int i = tid; i < tl.count * R_TOTAL; i += LORA_THREADS) {
    const int r = i / R_TOTAL, c = i % R_TOTAL;
    float v = part[r * LDW + c];
#pragma unroll
    for (int w = 1; w < LORA_WAVES; ++w) v += part[(w * 16 + r) * LDW + c];
    dst[i] = v;
  }
}

template <int R>
__global__ __launch_bounds__(LORA_THREADS) void lora_expand_add_kernel(
    unsigned short* __restrict__ out,       // [T, N] bf16, += in place
    const float* __restrict__ ws,           // [ksplit, Tl, P*R] f32
    const unsigned short* __restrict__ B,   // [S, N, R] bf16
    const int* __restrict__ row_idx, const int* __restrict__ tiles,
    int N, int T, int Tl, int S, int P, int seg1, int seg2, int ksplit) {
  constexpr int KS = R == 64 ? 2 : 1;  // MFMA k-steps per segment
  const LoraTile tl = lora_tile(tiles, blockIdx.x, S, Tl);
  if (tl.count <= 0) return;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int lc = lane & 15;
  const int lg = lane >> 4;

  int row = lc < tl.count ? row_idx[tl.first + lc] : -1;
  if (row >= T) row = -1;
  const bool live = row >= 0;
  // R == 16 fills half of the MFMA's K: lanes of the upper half hold zeros
  // on both operands
  const bool klive = R >= 32 || lg < 2;

  // h fragments: lane = h[row lc][p*R + ks*32 + lg*8 .. +8], summed over
  // the K splits in f32 and rounded once
  const int RT = P * R;
  u16x8 h0[KS], h1[KS], h2[KS];  // separate names: they stay in registers
  auto load_h = [&](int p, u16x8* hf) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live && klive && p < P) {
        const float* src =
            ws + (long)(tl.first + lc) * RT + p * R + ks * 32 + lg * 8;
        for (int kz = 0; kz < ksplit; ++kz) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(src);
          const f32x4 b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s[i] += a[i];
            s[4 + i] += b[i];
          }
          src += (long)Tl * RT;
        }
      }
      hf[ks] = f32_to_bf8(s);
    }
  };
  load_h(0, h0);
  load_h(1, h1);
  load_h(2, h2);

  const int nt0 = blockIdx.y * (LORA_NCHUNK / 16) + wave;
#pragma unroll
  for (int it = 0; it < LORA_NCHUNK / 16 / LORA_WAVES; ++it) {
    const int col0 = (nt0 + it * LORA_WAVES) * 16;
    if (col0 >= N) break;
    const int p = (col0 >= seg1) + (col0 >= seg2);  // wave-uniform
    const unsigned short* brow = B + ((long)tl.slot * N + col0 + lc) * R + lg * 8;
    f32x4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u16x8 bv = {0, 0, 0, 0, 0, 0, 0, 0};
      if (klive) bv = *reinterpret_cast<const u16x8*>(brow + ks * 32);
      const u16x8 hv = p == 0 ? h0[ks] : (p == 1 ? h1[ks] : h2[ks]);
      acc = lora_mfma(bv, hv, acc);  // D[col col0+lg*4+r][row lc]
    }
    if (live) {
      u16x4* o = reinterpret_cast<u16x4*>(out + (long)row * N + col0 + lg * 4);
      u16x4 ov = *o;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = f2bf(bf2f(ov[r]) + acc[r]);
      *o = ov;
    }
  }
}

template <int R_TOTAL>
void shrink_launch(float* ws, const void* x, const void* A, const int* row_idx,
                   const int* tiles, int ntiles, int ksplit, int K, int T,
                   int Tl, int S, hipStream_t s) {
  hipLaunchKernelGGL((lora_shrink_kernel<R_TOTAL>), dim3(ntiles, ksplit),
                     dim3(LORA_THREADS), 0, s, ws, (const unsigned short*)x,
                     (const unsigned short*)A, row_idx, tiles, K, T, Tl, S);
}

template <int R>
void expand_launch(void* out, const float* ws, const void* B,
                   const int* row_idx, const int* tiles, int ntiles, int N,
                   int T, int Tl, int S, int P, int seg1, int seg2, int ksplit,
                   hipStream_t s) {
  hipLaunchKernelGGL((lora_expand_add_kernel<R>),
                     dim3(ntiles, ceil_div(N, LORA_NCHUNK)),
                     dim3(LORA_THREADS), 0, s, (unsigned short*)out, ws,
                     (const unsigned short*)B, row_idx, tiles, N, T, Tl, S, P,
                     seg1, seg2, ksplit);
}

}  // namespace

// seg1/seg2: first output column of projection 1 / 2 (N where absent).
void lora_apply_launch(void* out, const void* x, const void* A, const void* B,
                       float* ws, const int* row_idx, const int* tiles,
                       int ntiles, int Tl, int T, int S, int K, int N, int P,
                       int R, int seg1, int seg2, int ksplit,
                       int* err_unsupported, hipStream_t s) {
  *err_unsupported = 0;
  const bool r_ok = R == 16 || R == 32 || R == 64;
  if (!r_ok || P < 1 || P > 3 || K % 64 != 0 || N % 16 != 0 || seg1 % 16 != 0 ||
      seg2 % 16 != 0 || ksplit < 1 || ksplit > 65535) {
    *err_unsupported = 1;
    return;
  }
  if (ntiles == 0) return;
#define LORA_SHRINK(RT)                                                     \
  case RT:                                                                  \
    shrink_launch<RT>(ws, x, A, row_idx, tiles, ntiles, ksplit, K, T, Tl, S, \
                      s);                                                   \
    break;
  switch (P * R) {
    LORA_SHRINK(16) LORA_SHRINK(32) LORA_SHRINK(48) LORA_SHRINK(64)
    LORA_SHRINK(96) LORA_SHRINK(128) LORA_SHRINK(192)
  }
#undef LORA_SHRINK
  if (R == 16)
    expand_launch<16>(out, ws, B, row_idx, tiles, ntiles, N, T, Tl, S, P, seg1,
                      seg2, ksplit, s);
  else if (R == 32)
    expand_launch<32>(out, ws, B, row_idx, tiles, ntiles, N, T, Tl, S, P, seg1,
                      seg2, ksplit, s);
  else
    expand_launch<64>(out, ws, B, row_idx, tiles, ntiles, N, T, Tl, S, P, seg1,
                      seg2, ksplit, s);
}
