// Grouped MoE expert GEMMs for MI355X (gfx950) — the sync-free dispatch
// path (round-2 item: remove the per-layer bincount/max host syncs and the
// padded-bmm overcompute so MoE decode can run under hipGraphs).
//
// Two kernels over the expert-sorted assignment list (sorting/count/offset
// tensors are computed on-device by moe_align in moe_route.hip, or by torch
// ops in models/llama.py MoEMLP where that kernel is switched off or out of
// range — no host readback anywhere):
//
//   moe_gate_up_silu: act[j, :] = silu(x[tok_j] @ Wg[e_j]^T) * (x[tok_j] @ Wu[e_j]^T)
//   moe_down_scale:   contrib[order[j], :] = (act[j] @ Wd[e_j]^T) * w_j
//
// GPT-OSS variants (per-expert biases + clamped swiglu, act_mode 1):
//   gate = min(g + bg, 7); up = clamp(u + bu, -7, 7)
//   act  = (up + 1) * gate * sigmoid(1.702 * gate)
//   contrib[order[j], :] = ((act[j] @ Wd[e_j]^T) + bd[e_j]) * w_j
// (matches models/llama.py MoEMLP._act_mul / the HF GptOss experts)
//
// Fixed launch grids (E x N-tiles) independent of the routing outcome:
// workgroups for empty experts exit immediately. MFMA 16x16x32 tiles,
// A = 16 gathered token rows staged through LDS in 512-element K chunks,
// B = expert weight panels streamed from HBM (read once per 16-row m-tile;
// typical decode occupancy is <= 2 m-tiles per expert).
#include "common.h"

namespace {

constexpr int MOE_BN = 64;        // N columns per workgroup (16 per wave)
constexpr int MOE_KC = 512;       // K chunk staged in LDS
constexpr int MOE_THREADS = 256;  // 4 waves

typedef __attribute__((ext_vector_type(8))) short m_s16x8;

DEVICE_INLINE f32x4 moe_mfma(u16x8 a, u16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(m_s16x8, a), __builtin_bit_cast(m_s16x8, b), c, 0, 0, 0);
}

// stage rows [16][kc] of gathered x into LDS (row padded to KC+8 elements
// to break the bank cycle on the A-frag reads)
template <bool GATHER>
DEVICE_INLINE void stage_rows(unsigned short* lds, const unsigned short* src,
                              long src_stride, const int* tok, int base_row,
                              int nrows, int k0, int kc, int tid) {
  const int units = 16 * (kc / 8);         // u16x8 units
  for (int u = tid; u < units; u += MOE_THREADS) {
    const int row = u / (kc / 8);
    const int kk = (u % (kc / 8)) * 8;
    u16x8 val = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < nrows) {
      const long r = GATHER ? (long)tok[row] : (long)(base_row + row);
      val = *reinterpret_cast<const u16x8*>(src + r * src_stride + k0 + kk);
    }
    *reinterpret_cast<u16x8*>(lds + row * (MOE_KC + 8) + kk) = val;
  }
}

// EXTM=false is the exact validated silu/no-bias fast path (identical to
// the r2-measured kernel); EXTM=true carries the GPT-OSS clamped-swiglu
// + expert-bias variant and only launches when those are requested.
template <bool EXTM = false>
__global__ __launch_bounds__(MOE_THREADS) void moe_gate_up_silu_kernel(
    unsigned short* __restrict__ act,       // [TK, I] bf16 (sorted rows)
    const unsigned short* __restrict__ x,   // [T, H] bf16
    const unsigned short* __restrict__ w,   // [E, 2I, H] bf16 (gate then up)
    const int* __restrict__ s_tok,          // [TK] token index per sorted row
    const int* __restrict__ offs,           // [E]
    const int* __restrict__ counts,         // [E]
    const unsigned short* __restrict__ bias,  // [E, 2I] bf16 or null
    int act_mode,                           // 0 = silu, 1 = clamped swiglu
    int H, int I) {
  const int nnt = I / MOE_BN;
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

  __shared__ unsigned short Xl[16 * (MOE_KC + 8)];

  const unsigned short* wg_panel =
      w + ((long)e * 2 * I + nt * MOE_BN + wave * 16) * H;
  const unsigned short* wu_panel =
      w + ((long)e * 2 * I + I + nt * MOE_BN + wave * 16) * H;

  // The kernel is weight-stream bound; a wave must keep enough loads in
  // flight to cover HBM latency (~600 ns). Weights are consumed in
  // K-blocks of 128 (4 MFMA k-steps), software-pipelined one block ahead:
  // 8 b128 loads (gate+up) issue while the previous block's 8 MFMAs run.
  const long wrow = (long)lc * H;  // this lane's weight row offset
  for (int m0 = 0; m0 < cnt; m0 += 16) {
    const int nrows = min(16, cnt - m0);
    f32x4 ag{0.f, 0.f, 0.f, 0.f}, au{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < H; k0 += MOE_KC) {
      const int kc = min(MOE_KC, H - k0);
      __syncthreads();
      stage_rows<true>(Xl, x, H, s_tok + base + m0, 0, nrows, k0, kc, tid);
      __syncthreads();
      // constexpr trip count on full chunks: the compiler fully unrolls
      // the 16 iterations and issues the 32 weight loads deep ahead of
      // the MFMAs (manual double-buffering with runtime-indexed register
      // arrays measured 10x SLOWER — selects, no unroll)
      auto body = [&](int kk) {
        const u16x8 a = *reinterpret_cast<const u16x8*>(
            Xl + lc * (MOE_KC + 8) + kk + lg * 8);
        const u16x8 g = *reinterpret_cast<const u16x8*>(
            wg_panel + wrow + k0 + kk + lg * 8);
        const u16x8 u = *reinterpret_cast<const u16x8*>(
            wu_panel + wrow + k0 + kk + lg * 8);
        ag = moe_mfma(a, g, ag);
        au = moe_mfma(a, u, au);
      };
      if (kc == MOE_KC) {
#pragma unroll
        for (int kk = 0; kk < MOE_KC; kk += 32) body(kk);
      } else {
        for (int kk = 0; kk < kc; kk += 32) body(kk);
      }
    }
    // D[row = lg*4 + r][col = lc]; fuse the activation and write.
    // EXTM: bias depends on the column only — one pair of loads per lane.
    float bg = 0.f, bu = 0.f;
    if constexpr (EXTM) {
      if (bias != nullptr) {
        const int col = nt * MOE_BN + wave * 16 + lc;
        bg = bf2f(bias[(long)e * 2 * I + col]);
        bu = bf2f(bias[(long)e * 2 * I + I + col]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = lg * 4 + r;
      if (row >= nrows) continue;
      float v;
      if (EXTM && act_mode == 1) {  // GPT-OSS clamped swiglu
        const float g = fminf(ag[r] + bg, 7.f);
        const float u = fminf(fmaxf(au[r] + bu, -7.f), 7.f);
        v = (u + 1.f) * g / (1.f + __expf(-1.702f * g));
      } else if constexpr (EXTM) {
        const float g = ag[r] + bg;
        v = g / (1.f + __expf(-g)) * (au[r] + bu);
      } else {
        const float g = ag[r];
        v = g / (1.f + __expf(-g)) * au[r];
      }
      act[(long)(base + m0 + row) * I + nt * MOE_BN + wave * 16 + lc] = f2bf(v);
    }
  }
}

template <bool EXTM = false>
__global__ __launch_bounds__(MOE_THREADS) void moe_down_scale_kernel(
    unsigned short* __restrict__ contrib,   // [TK, H] bf16 (original order)
    const unsigned short* __restrict__ act, // [TK, I] bf16 (sorted rows)
    const unsigned short* __restrict__ w,   // [E, H, I] bf16
    const int* __restrict__ offs,           // [E]
    const int* __restrict__ counts,         // [E]
    const int* __restrict__ order,          // [TK] sorted -> original index
    const float* __restrict__ flat_w,       // [TK] routing weight (original)
    const unsigned short* __restrict__ bias,  // [E, H] bf16 or null
    int H, int I) {
  const int nnt = H / MOE_BN;
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

  __shared__ unsigned short Al[16 * (MOE_KC + 8)];

  const unsigned short* wd_panel =
      w + ((long)e * H + nt * MOE_BN + wave * 16) * I;
  const int first = base;  // act rows are consecutive in sorted space

  const long wrow = (long)lc * I;
  for (int m0 = 0; m0 < cnt; m0 += 16) {
    const int nrows = min(16, cnt - m0);
    f32x4 acc{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < I; k0 += MOE_KC) {
      const int kc = min(MOE_KC, I - k0);
      __syncthreads();
      stage_rows<false>(Al, act, I, nullptr, first + m0, nrows, k0, kc, tid);
      __syncthreads();
      auto body = [&](int kk) {
        const u16x8 a = *reinterpret_cast<const u16x8*>(
            Al + lc * (MOE_KC + 8) + kk + lg * 8);
        const u16x8 b = *reinterpret_cast<const u16x8*>(
            wd_panel + wrow + k0 + kk + lg * 8);
        acc = moe_mfma(a, b, acc);
      };
      if (kc == MOE_KC) {
#pragma unroll
        for (int kk = 0; kk < MOE_KC; kk += 32) body(kk);
      } else {
        for (int kk = 0; kk < kc; kk += 32) body(kk);
      }
    }
    float bd = 0.f;
    if constexpr (EXTM) {
      bd = (bias != nullptr)
          ? bf2f(bias[(long)e * H + nt * MOE_BN + wave * 16 + lc]) : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = lg * 4 + r;
      if (row >= nrows) continue;
      const int oj = order[base + m0 + row];
      if constexpr (EXTM) {
        contrib[(long)oj * H + nt * MOE_BN + wave * 16 + lc] =
            f2bf((acc[r] + bd) * flat_w[oj]);
      } else {
        contrib[(long)oj * H + nt * MOE_BN + wave * 16 + lc] =
            f2bf(acc[r] * flat_w[oj]);
      }
    }
  }
}

}  // namespace

void moe_gate_up_silu_launch(void* act, const void* x, const void* w,
                             const int* s_tok, const int* offs,
                             const int* counts, const void* bias,
                             int act_mode, int E, int H, int I,
                             int* err_unsupported, hipStream_t s) {
  *err_unsupported = 0;
  if (I % MOE_BN != 0 || H % 128 != 0) { *err_unsupported = 1; return; }
  dim3 grid(E * (I / MOE_BN));
  const bool extm = bias != nullptr || act_mode != 0;
  if (extm)
    hipLaunchKernelGGL((moe_gate_up_silu_kernel<true>), grid,
                       dim3(MOE_THREADS), 0, s, (unsigned short*)act,
                       (const unsigned short*)x, (const unsigned short*)w,
                       s_tok, offs, counts, (const unsigned short*)bias,
                       act_mode, H, I);
  else
    hipLaunchKernelGGL((moe_gate_up_silu_kernel<false>), grid,
                       dim3(MOE_THREADS), 0, s, (unsigned short*)act,
                       (const unsigned short*)x, (const unsigned short*)w,
                       s_tok, offs, counts, (const unsigned short*)bias,
                       act_mode, H, I);
}

void moe_down_scale_launch(void* contrib, const void* act, const void* w,
                           const int* offs, const int* counts,
                           const int* order, const float* flat_w,
                           const void* bias, int E,
                           int H, int I, int* err_unsupported, hipStream_t s) {
  *err_unsupported = 0;
  if (H % MOE_BN != 0 || I % 128 != 0) { *err_unsupported = 1; return; }
  dim3 grid(E * (H / MOE_BN));
  if (bias != nullptr)
    hipLaunchKernelGGL((moe_down_scale_kernel<true>), grid,
                       dim3(MOE_THREADS), 0, s, (unsigned short*)contrib,
                       (const unsigned short*)act, (const unsigned short*)w,
                       offs, counts, order, flat_w,
                       (const unsigned short*)bias, H, I);
  else
    hipLaunchKernelGGL((moe_down_scale_kernel<false>), grid,
                       dim3(MOE_THREADS), 0, s, (unsigned short*)contrib,
                       (const unsigned short*)act, (const unsigned short*)w,
                       offs, counts, order, flat_w,
                       (const unsigned short*)bias, H, I);
}
