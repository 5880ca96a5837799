// Paged-attention decode for MI355X (gfx950) — the TPOT-dominant kernel.
//
// Single new token per sequence attends over the paged KV cache.
// Replaces what the reference delegates to vLLM's paged_attention kernels
// (SURVEY.md §2.9 #1); designed for CDNA4 rather than ported:
//
//  - one workgroup per (sequence, kv_head); GQA q-heads (GQ = Hq/Hkv) share
//    the K/V stream so each KV byte is read exactly once per step.
//  - 4 waves * 4 lane-groups of 16 = 16 independent online-softmax streams;
//    a 16-lane group owns one token per iteration, lane = 8 head dims
//    (16 B = u16x8 loads -> 1 KiB per wave per iteration, fully coalesced
//    against the [block, kv_head, block_size, D] pool layout).
//  - streams merge via 64-wide shuffles (cross-group) then LDS (cross-wave);
//    accumulation entirely in f32.
//
// KV pool layout: [num_blocks, Hkv, BS, D] bf16, BS = 16 tokens.
#include "common.h"

#include <type_traits>

namespace {

constexpr int BS = 16;       // tokens per KV block (page)
constexpr int NWAVES = 4;    // waves per workgroup
constexpr int THREADS = NWAVES * WAVE_SIZE;

// Arguments only the fused kernels have (rope + cache write folded in).
struct FusedDecodeArgs {
  const long* positions;        // [N]
  const float* cos_sin;         // [max_pos, D] f32: D/2 cos then D/2 sin
  const unsigned short* k;      // [N, Hkv, D] new-token rows (qkv view)
  const unsigned short* v;
  long k_stride, v_stride;      // row strides (elements)
  const long* slot_mapping;     // [N] block*BS + offset, < 0 = no write
};

// One lane's 8 dims of a NeoX-roped head row. The 16 lanes of a group hold
// dims [8*sub, 8*sub+8), so the rotate-half partner sits 8 lanes away
// (row_ror:8 of the packed row). co/si are this lane's 8 cos / sin values.
// Same f32 expressions and the same single rounding as rope_neox_kernel:
// first half x1*co - x2*si, second half x2*co + x1*si, written with the
// contraction that kernel compiles to so both stay bit-identical.
DEVICE_INLINE u16x8 rope_neox_lane(u16x8 own, const float* co, const float* si,
                                   bool second_half) {
  u32x4 ow = __builtin_bit_cast(u32x4, own), pw;
#pragma unroll
  for (int i = 0; i < 4; ++i) pw[i] = dpp_row_ror<8>(ow[i]);
  const u16x8 oth = __builtin_bit_cast(u16x8, pw);
  u16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float cross = bf2f(oth[i]) * si[i];
    r[i] = f2bf(__builtin_fmaf(bf2f(own[i]), co[i],
                               second_half ? cross : -cross));
  }
  return r;
}

// new token's roped K and plain V, one 16 B slice per `sub`
__shared__ u16x8 lds_new_token[2][16];

// Where the new token sits in the sequence (-1: it was not written), and
// how the lane group that meets that position in its page stream gets its
// K/V: from the LDS copy, never from the pool, where this workgroup's own
// store may not have landed yet.
struct NewToken {
  int pos;
  DEVICE_INLINE void take(u16x8& k, u16x8& v, int sub) const {
    k = lds_new_token[0][sub];
    v = lds_new_token[1][sub];
  }
};

// What rope_neox_kernel and reshape_and_cache_kernel do for this
// workgroup's rows of a plain decode step (D=128, bf16 pools): rope the GQ
// packed q rows in registers, rope the new token's K, and store it with V
// to `slot` — one lane group per workgroup writes, slot < 0 writes nothing.
// The caller's contract is that of the engine's decode step: the row's new
// token is position len-1 of its sequence and slot is that position's place
// in the block table. The values and the order of every operation are those
// of the three-kernel sequence.
template <int GQ>
DEVICE_INLINE NewToken fused_prologue(const FusedDecodeArgs& fa,
                                      u16x8 (&qb)[GQ][1], const void* kc,
                                      const void* vc, int seq, int h, int Hkv,
                                      int len) {
  constexpr int D = 128;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int sub = lane & 15;
  const long slot = fa.slot_mapping[seq];
  const float* cs = fa.cos_sin + fa.positions[seq] * D + (sub & 7) * 8;
  float co[8], si[8];
#pragma unroll
  for (int i = 0; i < 8; i += 4) {
    *reinterpret_cast<f32x4*>(co + i) = *reinterpret_cast<const f32x4*>(cs + i);
    *reinterpret_cast<f32x4*>(si + i) =
        *reinterpret_cast<const f32x4*>(cs + D / 2 + i);
  }
  const long hoff = (long)h * D + sub * 8;
  const u16x8 kraw =
      *reinterpret_cast<const u16x8*>(fa.k + (long)seq * fa.k_stride + hoff);
  const u16x8 vnew =
      *reinterpret_cast<const u16x8*>(fa.v + (long)seq * fa.v_stride + hoff);
#pragma unroll
  for (int gq = 0; gq < GQ; ++gq)
    qb[gq][0] = rope_neox_lane(qb[gq][0], co, si, sub >= 8);
  const u16x8 knew = rope_neox_lane(kraw, co, si, sub >= 8);
  if (wave == 0 && lane < 16) {
    lds_new_token[0][sub] = knew;
    lds_new_token[1][sub] = vnew;
    if (slot >= 0) {
      const long dst = ((slot / BS * Hkv + h) * BS + slot % BS) * D + sub * 8;
      // the pools are writable on this path (the launcher passes them
      // non-const); every other access in the kernel only reads them
      *reinterpret_cast<u16x8*>((unsigned short*)kc + dst) = knew;
      *reinterpret_cast<u16x8*>((unsigned short*)vc + dst) = vnew;
    }
  }
  __syncthreads();
  return NewToken{slot >= 0 ? len - 1 : -1};
}

// Group sum of d*scale over a 16-lane group with DPP instead of the LDS
// crossbar: a group is one DPP row and every lane reads exactly the lane the
// xor butterfly of group16_reduce_sum reads (i^8, i^4, i^2, i^1). The first butterfly step is the fma the shuffle version of these
// kernels has always been compiled to: fma(d, scale, partner's rounded
// d*scale). After it the two partners no longer hold the same value, which
// is why the lanes pair up exactly as in the xor butterfly.
DEVICE_INLINE float group16_sum_scaled_dpp(float d, float scale) {
  float x = d * scale;
  x = __builtin_fmaf(d, scale,
                     __uint_as_float(dpp_row_xor<8>(__float_as_uint(x))));
  x += __uint_as_float(dpp_row_xor<4>(__float_as_uint(x)));
  x += __uint_as_float(dpp_row_xor<2>(__float_as_uint(x)));
  x += __uint_as_float(dpp_row_xor<1>(__float_as_uint(x)));
  return x;
}

// The same decode step for the serving fast path, D=128 bf16 at GQ 4 and 5
// (two tokens per group and softmax update), rescheduled:
//  - the 16-lane dot reduce runs on DPP;
//  - the block-table entry of the wave's next page is fetched a page ahead;
//  - at GQ 4 the K/V stage (2 tokens x K,V = 16 VGPRs) is double-buffered:
//    the next stage's loads are issued before the current one is computed,
//    so loads stay in flight across the compute (at GQ 5 the second stage
//    would cost a wave per SIMD, and measured slower). Only entries and
//    stages of pages < npages are ever touched.
// Every f32 operation and its order are those of paged_attn_decode_body at
// these GQ. Its sums with two candidate products for an fma are uniform there
// and written out with fmaf here, so the results are the same to the bit
// (checked on 2-2.6 M outputs per GQ, profiles/decode_fused.md).
template <int GQ, bool FUSED>
DEVICE_INLINE void paged_attn_decode_fast_body(
    unsigned short* __restrict__ out, const unsigned short* __restrict__ q,
    const void* kc, const void* vc, const int* __restrict__ block_tables,
    const int* __restrict__ seq_lens, int Hkv, int max_blocks, float scale,
    long q_stride, const FusedDecodeArgs& fa) {
  static_assert(GQ == 4 || GQ == 5, "pinned against the GQ 4/5 kernels only");
  constexpr int D = 128, DV = 8, TB = 2;
  constexpr bool PREFETCH = GQ == 4;

  const int seq = blockIdx.x;
  const int h = blockIdx.y;        // kv head
  const int Hq = Hkv * GQ;
  const int len = seq_lens[seq];
  const int npages = (len + BS - 1) / BS;

  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int g = lane >> 4;         // token-group within wave [0,4)
  const int sub = lane & 15;       // dim-slice within group [0,16)

  u16x8 qb[GQ][1];                 // q stays packed for v_dot2c
#pragma unroll
  for (int gq = 0; gq < GQ; ++gq)
    qb[gq][0] = *reinterpret_cast<const u16x8*>(
        q + (long)seq * q_stride + ((long)h * GQ + gq) * D + sub * DV);

  [[maybe_unused]] NewToken nt;
  if constexpr (FUSED) nt = fused_prologue<GQ>(fa, qb, kc, vc, seq, h, Hkv, len);

  float m[GQ], s[GQ], acc[GQ][DV];
#pragma unroll
  for (int gq = 0; gq < GQ; ++gq) {
    m[gq] = -INFINITY;
    s[gq] = 0.f;
#pragma unroll
    for (int j = 0; j < DV; ++j) acc[gq][j] = 0.f;
  }

  const int* bt = block_tables + (long)seq * max_blocks;
  struct Stage {
    u16x8 k[TB], v[TB];
  };
  auto issue = [&](Stage& st, int blk, int tb) {
    const unsigned short* kbase =
        (const unsigned short*)kc + (((long)blk * Hkv + h) * BS) * D;
    const unsigned short* vbase =
        (const unsigned short*)vc + (((long)blk * Hkv + h) * BS) * D;
#pragma unroll
    for (int it = 0; it < TB; ++it) {
      const int tok = (tb + it) * 4 + g;
      st.k[it] = *reinterpret_cast<const u16x8*>(kbase + tok * D + sub * DV);
      st.v[it] = *reinterpret_cast<const u16x8*>(vbase + tok * D + sub * DV);
    }
  };

  int page = wave;
  int blk = 0;
  Stage cur;
  if (page < npages) {
    blk = bt[page];
    if constexpr (PREFETCH) issue(cur, blk, 0);
  }
  while (page < npages) {
    const int next_page = page + NWAVES;
    const bool more = next_page < npages;
    int next_blk = 0;
    if (more) next_blk = bt[next_page];
#pragma unroll
    for (int tb = 0; tb < BS / 4; tb += TB) {
      Stage nxt;
      if constexpr (!PREFETCH) {
        issue(cur, blk, tb);
      } else if (tb + TB < BS / 4) {
        issue(nxt, blk, tb + TB);
      } else if (more) {
        issue(nxt, next_blk, 0);
      }
      const int base_tok = page * BS + tb * 4 + g;
      if constexpr (FUSED) {
#pragma unroll
        for (int it = 0; it < TB; ++it)
          if (nt.pos == base_tok + it * 4) nt.take(cur.k[it], cur.v[it], sub);
      }
#pragma unroll
      for (int gq = 0; gq < GQ; ++gq) {
        float dot[TB];
#pragma unroll
        for (int it = 0; it < TB; ++it) {
          float d = 0.f;
          const bf16x2* qa = reinterpret_cast<const bf16x2*>(&qb[gq][0]);
          const bf16x2* ka = reinterpret_cast<const bf16x2*>(&cur.k[it]);
#pragma unroll
          for (int j = 0; j < DV / 2; ++j)
            d = __builtin_amdgcn_fdot2_f32_bf16(qa[j], ka[j], d, false);
          dot[it] = d;
        }
#pragma unroll
        for (int it = 0; it < TB; ++it)  // all 16 lanes get the scaled dot
          dot[it] = group16_sum_scaled_dpp(dot[it], scale);
        float pmax = -INFINITY;
#pragma unroll
        for (int it = 0; it < TB; ++it) {
          const bool valid = base_tok + it * 4 < len;
          dot[it] = valid ? dot[it] : -INFINITY;
          pmax = fmaxf(pmax, dot[it]);
        }
        if (pmax == -INFINITY) continue;
        const float nm = fmaxf(m[gq], pmax);
        const float corr = __expf(m[gq] - nm);  // exp(-inf - finite) = 0
        float p[TB];
        float psum = 0.f;
#pragma unroll
        for (int it = 0; it < TB; ++it) {
          p[it] = (dot[it] == -INFINITY) ? 0.f : __expf(dot[it] - nm);
          psum += p[it];
        }
        s[gq] = s[gq] * corr + psum;
#pragma unroll
        for (int j = 0; j < DV; ++j) {
          // acc*corr + p0*v0 + p1*v1: p0*v0 is the product that is rounded
          float a = __builtin_fmaf(acc[gq][j], corr, p[0] * bf2f(cur.v[0][j]));
          acc[gq][j] = __builtin_fmaf(p[1], bf2f(cur.v[1][j]), a);
        }
        m[gq] = nm;
      }
      if constexpr (PREFETCH) cur = nxt;
    }
    page = next_page;
    blk = next_blk;
  }

  // Merge the 4 token-group streams within each wave (butterfly over
  // lane masks 16 and 32). Lanes with equal `sub` end up identical.
#pragma unroll
  for (int mask = 16; mask <= 32; mask <<= 1) {
#pragma unroll
    for (int gq = 0; gq < GQ; ++gq) {
      const float om = __shfl_xor(m[gq], mask, WAVE_SIZE);
      const float os = __shfl_xor(s[gq], mask, WAVE_SIZE);
      float oacc[DV];
#pragma unroll
      for (int j = 0; j < DV; ++j)
        oacc[j] = __shfl_xor(acc[gq][j], mask, WAVE_SIZE);
      const float nm = fmaxf(m[gq], om);
      if (os > 0.f || s[gq] > 0.f) {
        const float w1 = (s[gq] > 0.f) ? __expf(m[gq] - nm) : 0.f;
        const float w2 = (os > 0.f) ? __expf(om - nm) : 0.f;
        // s*w1 + os*w2 rounds os*w2; acc*w1 + oacc*w2 rounds acc*w1
        s[gq] = __builtin_fmaf(s[gq], w1, os * w2);
#pragma unroll
        for (int j = 0; j < DV; ++j)
          acc[gq][j] = __builtin_fmaf(oacc[j], w2, acc[gq][j] * w1);
        m[gq] = nm;
      }
    }
  }

  // Cross-wave merge through LDS.
  __shared__ float lds_acc[NWAVES][GQ][D];
  __shared__ float lds_m[NWAVES][GQ];
  __shared__ float lds_s[NWAVES][GQ];
  if (g == 0) {  // one representative lane-group per wave
#pragma unroll
    for (int gq = 0; gq < GQ; ++gq) {
#pragma unroll
      for (int j = 0; j < DV; ++j) lds_acc[wave][gq][sub * DV + j] = acc[gq][j];
      if (sub == 0) {
        lds_m[wave][gq] = m[gq];
        lds_s[wave][gq] = s[gq];
      }
    }
  }
  __syncthreads();

  // 256 threads cover (gq, d) output elements.
  for (int u = threadIdx.x; u < GQ * D; u += THREADS) {
    const int gq = u / D;
    const int d = u % D;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w)
      if (lds_s[w][gq] > 0.f) M = fmaxf(M, lds_m[w][gq]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
      if (lds_s[w][gq] > 0.f) {
        const float wt = __expf(lds_m[w][gq] - M);
        num += wt * lds_acc[w][gq][d];
        den += wt * lds_s[w][gq];
      }
    }
    out[((long)seq * Hq + (long)h * GQ + gq) * D + d] =
        f2bf(den > 0.f ? num / den : 0.f);
  }
}

// GQ 4 and 5 of the D=128 bf16 fast path take the rescheduled body.
template <int D, int GQ, bool FP8, bool EXT>
constexpr bool kDecodeFast = D == 128 && !FP8 && !EXT && (GQ == 4 || GQ == 5);

// <128, 5> sits right on the 128-VGPR line: asked for 4 waves per SIMD it
// fits in 128 registers without scratch, as the kernel always did.
template <int D, int GQ, bool FP8, bool EXT = false>
__global__ __launch_bounds__(THREADS, (kDecodeFast<D, GQ, FP8, EXT> && GQ == 5) ? 4 : 1)
void paged_attn_decode_kernel(
    unsigned short* __restrict__ out,        // [N, Hq, D]
    const unsigned short* __restrict__ q,    // [N, Hq, D]
    const void* __restrict__ kc,             // [B, Hkv, BS, D] bf16|fp8
    const void* __restrict__ vc,             // [B, Hkv, BS, D]
    const int* __restrict__ block_tables,    // [N, max_blocks]
    const int* __restrict__ seq_lens,        // [N]
    int Hkv, int max_blocks, float scale, long q_stride,
    const float* __restrict__ sinks,         // [Hq] or null (GPT-OSS)
    int window,                              // 0 = full attention
    float softcap) {                         // 0 = off (Gemma-2 tanh cap)
  if constexpr (kDecodeFast<D, GQ, FP8, EXT>) {
    paged_attn_decode_fast_body<GQ, false>(out, q, kc, vc, block_tables,
                                           seq_lens, Hkv, max_blocks, scale,
                                           q_stride, FusedDecodeArgs{});
  } else {
#define DECODE_BODY_FUSED 0
#include "attn_decode_body.h"
#undef DECODE_BODY_FUSED
  }
}

// Plain decode step (every row the one new token of a distinct sequence):
// rope, KV-cache write and attention in one launch over the same body as
// the plain kernel of that GQ. q/k/v are the unroped rows of the qkv
// buffer, which is left as it is.
template <int D, int GQ, bool FP8 = false>
__global__ __launch_bounds__(THREADS) void paged_attn_decode_fused_kernel(
    unsigned short* __restrict__ out,        // [N, Hq, D]
    const unsigned short* __restrict__ q,    // [N, Hq, D] unroped
    unsigned short* kc,                      // [B, Hkv, BS, D] bf16, written
    unsigned short* vc,
    const int* __restrict__ block_tables,    // [N, max_blocks]
    const int* __restrict__ seq_lens,        // [N], new token included
    int Hkv, int max_blocks, float scale, long q_stride,
    FusedDecodeArgs fa) {
  static_assert(D == 128 && !FP8, "fused decode covers D=128 bf16 pools");
  if constexpr (kDecodeFast<D, GQ, FP8, false>) {
    paged_attn_decode_fast_body<GQ, true>(out, q, kc, vc, block_tables,
                                          seq_lens, Hkv, max_blocks, scale,
                                          q_stride, fa);
  } else {
    constexpr bool EXT = false;  // the body's feature arguments, all off
    [[maybe_unused]] const float* sinks = nullptr;
    [[maybe_unused]] const int window = 0;
    [[maybe_unused]] const float softcap = 0.f;
#define DECODE_BODY_FUSED 1
#include "attn_decode_body.h"
#undef DECODE_BODY_FUSED
  }
}

}  // namespace

void paged_attn_decode_launch(void* out, const void* q, const void* kc,
                              const void* vc, const int* block_tables,
                              const int* seq_lens, int N, int Hq, int Hkv,
                              int D, int max_blocks, float scale, long q_stride,
                              int fp8, const float* sinks, int window,
                              float softcap, int* err_unsupported,
                              hipStream_t s) {
  const int GQ = Hq / Hkv;
  dim3 grid(N, Hkv);
  dim3 block(THREADS);
  *err_unsupported = 0;
  if (D != 128 && D != 64 && D != 256) { *err_unsupported = 1; return; }
  if (D == 256 && GQ > 4) { *err_unsupported = 1; return; }  // VGPR budget
  const bool ext = (sinks != nullptr) || window > 0 || softcap > 0.f;
#define LAUNCH_D(DD, G, F, E)                                                  \
  hipLaunchKernelGGL((paged_attn_decode_kernel<DD, G, F, E>), grid, block, 0,  \
                     s, (unsigned short*)out, (const unsigned short*)q, kc,    \
                     vc, block_tables, seq_lens, Hkv, max_blocks, scale,       \
                     q_stride, sinks, window, softcap)
#define LAUNCH_GQ2(G, F)                                                       \
  do {                                                                         \
    if (D == 128) {                                                            \
      if (ext) LAUNCH_D(128, G, F, true);                                      \
      else LAUNCH_D(128, G, F, false);                                         \
    } else if (D == 64) {                                                      \
      LAUNCH_D(64, G, F, true);                                                \
    } else if ((G) <= 4) {                                                     \
      LAUNCH_D(256, (G) <= 4 ? (G) : 1, F, true);                              \
    }                                                                          \
  } while (0)
#define LAUNCH_GQ(G)                                                          \
  do {                                                                        \
    if (fp8) LAUNCH_GQ2(G, true);                                             \
    else LAUNCH_GQ2(G, false);                                                \
  } while (0)
  switch (GQ) {
    case 1: LAUNCH_GQ(1); break;
    case 2: LAUNCH_GQ(2); break;
    case 4: LAUNCH_GQ(4); break;
    case 5: LAUNCH_GQ(5); break;
    case 6: LAUNCH_GQ(6); break;
    case 7: LAUNCH_GQ(7); break;
    case 8: LAUNCH_GQ(8); break;
    default: *err_unsupported = 1; return;
  }
#undef LAUNCH_GQ
#undef LAUNCH_GQ2
#undef LAUNCH_D
}

void paged_attn_decode_fused_launch(
    void* out, const void* q, const void* k, const void* v, void* kc, void* vc,
    const long* positions, const float* cos_sin, const long* slot_mapping,
    const int* block_tables, const int* seq_lens, int N, int Hq, int Hkv,
    int D, int max_blocks, float scale, long q_stride, long k_stride,
    long v_stride, int* err_unsupported, hipStream_t s) {
  const int GQ = Hq / Hkv;
  dim3 grid(N, Hkv);
  dim3 block(THREADS);
  *err_unsupported = 0;
  if (D != 128) { *err_unsupported = 1; return; }
  const FusedDecodeArgs fa{positions, cos_sin, (const unsigned short*)k,
                           (const unsigned short*)v, k_stride, v_stride,
                           slot_mapping};
#define LAUNCH_FUSED(G)                                                        \
  hipLaunchKernelGGL((paged_attn_decode_fused_kernel<128, G>), grid, block, 0, \
                     s, (unsigned short*)out, (const unsigned short*)q,        \
                     (unsigned short*)kc, (unsigned short*)vc, block_tables,   \
                     seq_lens, Hkv, max_blocks, scale, q_stride, fa)
  switch (GQ) {
    case 1: LAUNCH_FUSED(1); break;
    case 2: LAUNCH_FUSED(2); break;
    case 4: LAUNCH_FUSED(4); break;
    case 5: LAUNCH_FUSED(5); break;
    case 6: LAUNCH_FUSED(6); break;
    case 7: LAUNCH_FUSED(7); break;
    case 8: LAUNCH_FUSED(8); break;
    default: *err_unsupported = 1; return;
  }
#undef LAUNCH_FUSED
}
