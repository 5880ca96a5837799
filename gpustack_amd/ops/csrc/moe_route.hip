// MoE routing for MI355X (gfx950): everything between the router logits and
// the grouped expert GEMMs of moe_gemm.hip, in two launches.
//
//   moe_route: logits [T, E] f32 -> experts [T, k] i32, weights [T, k] f32
//   moe_align: experts [T*k]     -> s_tok, order [T*k], offs, counts [E] i32
//
// moe_route. One wave routes one token (4 waves per block, no LDS, no
// barrier, no atomic). Lane l holds the experts l, l+64, ... in registers
// (VPL values per lane). Selection is k rounds of a wave-wide max over a
// 64-bit key: the high word is the order-preserving integer image of the f32
// value, the low word the complemented index, so "larger value first, lower
// index on equal values" is a plain unsigned compare and the winner's value
// and index both come back out of the key. The butterfly's four steps inside
// a 16-lane row are DPP operand selects; the two steps across rows go through
// the LDS crossbar (__shfl_xor). Key 0 marks a taken, masked or out-of-range
// slot: every real key is larger, so an index >= E is never selected.
//
//   softmax, renorm     w = softmax over the k selected logits
//   softmax, no renorm  w = full-softmax probability of the selected experts
//   sigmoid_bias        s = sigmoid(logit), choice = s + bias; with n_group
//                       > 1 a group scores the sum of its two largest choices
//                       and only the topk_group best groups stay eligible;
//                       w = s at the selected experts, / (sum + 1e-20) when
//                       renormalised, * scale
//
// A group is a run of E/n_group consecutive experts. The kernel takes group
// sizes that divide 64: a group is then an aligned run of lanes of one
// register slot, its top-2 is an xor butterfly over (max, second max) pairs
// that stays inside the run, and the groups are ranked by the same key-max.
// Every exponential takes an argument <= 0.
//
// moe_align. One block per expert, so the grid depends on E alone and the
// launch is the same for any T (hipGraph-capturable). Block e walks the flat
// assignment list in 64-wide chunks; a ballot per chunk counts the entries
// < e (their total is offs[e]) and == e (counts[e]). The 4 waves take
// disjoint contiguous ranges of chunks and exchange their two counts through
// LDS. A second walk writes order/s_tok for the block's own entries at
// offs[e] + entries of e in earlier chunks + ballot prefix popcount: the
// position in a stable sort. No block waits on another and nothing is
// atomic, so the result is deterministic. Every write lands below
// count(< e) + count(== e) <= T*k whatever the list holds.
#include <limits.h>

#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int ROUTE_WAVES = 4;
constexpr int ALIGN_WAVES = 4;
constexpr int ALIGN_UNROLL = 4;  // chunk loads in flight per wave

// f32 -> u32 with the order of the float values (-0 == +0).
DEVICE_INLINE unsigned ord32(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEVICE_INLINE float unord32(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

DEVICE_INLINE u64 make_key(float v, int idx) {
  return ((u64)ord32(v) << 32) | (unsigned)~idx;
}

DEVICE_INLINE int key_index(u64 key) { return (int)~(unsigned)key; }

DEVICE_INLINE u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

template <int M>
DEVICE_INLINE u64 dpp_xor64(u64 x) {
  return ((u64)dpp_row_xor<M>((unsigned)(x >> 32)) << 32) |
         dpp_row_xor<M>((unsigned)x);
}

DEVICE_INLINE u64 shfl_xor64(u64 x, int m) {
  return ((u64)__shfl_xor((unsigned)(x >> 32), m, WAVE_SIZE) << 32) |
         (unsigned)__shfl_xor((unsigned)x, m, WAVE_SIZE);
}

// Max of a 64-bit key over the wave, in every lane.
DEVICE_INLINE u64 wave_max_key(u64 x) {
  x = umax64(x, dpp_xor64<1>(x));
  x = umax64(x, dpp_xor64<2>(x));
  x = umax64(x, dpp_xor64<4>(x));
  x = umax64(x, dpp_xor64<8>(x));
  x = umax64(x, shfl_xor64(x, 16));
  x = umax64(x, shfl_xor64(x, 32));
  return x;
}

// exp(x)/(1 + exp(x)) with the exponential taken at -|x|.
DEVICE_INLINE float sigmoid_f32(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.f ? 1.f : e) / (1.f + e);
}

template <int VPL>
DEVICE_INLINE u64 local_max(const u64 (&key)[VPL]) {
  u64 best = key[0];
#pragma unroll
  for (int j = 1; j < VPL; ++j) best = umax64(best, key[j]);
  return best;
}

// Leave only the experts of the topk_group best groups eligible: the others
// get choice = -inf. gshift = log2(group size), group size divides 64.
template <int VPL>
DEVICE_INLINE void keep_best_groups(float (&c)[VPL], int lane, int E,
                                    int gshift, int topk_group) {
  const int gsz = 1 << gshift;
  u64 gkey[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    float m1 = c[j], m2 = -INFINITY;  // two largest of the lane's run
    for (int m = 1; m < gsz; m <<= 1) {
      const float o1 = __shfl_xor(m1, m, WAVE_SIZE);
      const float o2 = __shfl_xor(m2, m, WAVE_SIZE);
      m2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
      m1 = fmaxf(m1, o1);
    }
    const int idx = lane + WAVE_SIZE * j;
    gkey[j] = idx < E ? make_key(m1 + m2, idx >> gshift) : 0;
  }
  unsigned keep = 0;
  for (int r = 0; r < topk_group; ++r) {
    const int g = key_index(wave_max_key(local_max(gkey)));
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      if (gkey[j] != 0 && ((lane + WAVE_SIZE * j) >> gshift) == g) {
        keep |= 1u << j;
        gkey[j] = 0;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPL; ++j)
    if (!((keep >> j) & 1u)) c[j] = -INFINITY;
}

template <int VPL, bool SIGMOID>
__global__ void __launch_bounds__(ROUTE_WAVES* WAVE_SIZE)
moe_route_kernel(int* __restrict__ experts, float* __restrict__ weights,
                 const float* __restrict__ logits,
                 const float* __restrict__ bias, int T, int E, int k,
                 int renorm, int gshift, int n_group, int topk_group,
                 float scale) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int t = blockIdx.x * ROUTE_WAVES + (threadIdx.x >> 6);
  if (t >= T) return;  // whole waves leave: the ones that stay are full
  const float* row = logits + (long)t * E;

  float c[VPL];  // the value that selects
  float s[VPL];  // sigmoid score (SIGMOID only)
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int idx = lane + WAVE_SIZE * j;
    c[j] = idx < E ? row[idx] : -INFINITY;
    if constexpr (SIGMOID) {
      s[j] = sigmoid_f32(c[j]);
      if (idx < E) c[j] = s[j] + (bias ? bias[idx] : 0.f);
    }
  }
  if constexpr (SIGMOID) {
    if (n_group > 1 && topk_group < n_group)
      keep_best_groups<VPL>(c, lane, E, gshift, topk_group);
  }

  u64 key[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j)
    key[j] = lane + WAVE_SIZE * j < E ? make_key(c[j], lane + WAVE_SIZE * j) : 0;

  // lane r keeps the result of round r
  int my_idx = 0;
  float my_val = -INFINITY;  // selected logit (softmax) or score (sigmoid)
  float top = 0.f;           // round 0's value: the row maximum
  for (int r = 0; r < k; ++r) {
    const u64 win = wave_max_key(local_max(key));
    const int idx = key_index(win);
    float val = unord32((unsigned)(win >> 32));
    if constexpr (SIGMOID) {
      float sj = 0.f;
#pragma unroll
      for (int j = 0; j < VPL; ++j)
        if ((idx >> 6) == j) sj = s[j];
      val = __shfl(sj, idx & (WAVE_SIZE - 1), WAVE_SIZE);
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j)
      if (lane + WAVE_SIZE * j == idx) key[j] = 0;
    if (r == 0) top = val;
    if (lane == r) {
      my_idx = idx;
      my_val = val;
    }
  }

  float w;
  if constexpr (SIGMOID) {
    w = lane < k ? my_val : 0.f;
    if (renorm) w = w / (wave_reduce_sum(w) + 1e-20f);
    w *= scale;
  } else {
    w = lane < k ? expf(my_val - top) : 0.f;
    float den = w;
    if (!renorm) {
      den = 0.f;
#pragma unroll
      for (int j = 0; j < VPL; ++j)
        if (lane + WAVE_SIZE * j < E) den += expf(c[j] - top);
    }
    w = w / wave_reduce_sum(den);
  }
  if (lane < k) {
    experts[(long)t * k + lane] = my_idx;
    weights[(long)t * k + lane] = w;
  }
}

// Walks the chunks [c0, c1) of the list, ALIGN_UNROLL loads ahead of their
// use, and calls f(first entry index of the chunk, the lane's entry); lanes
// past the end of the list see INT_MAX.
template <class F>
DEVICE_INLINE void for_chunks(const int* __restrict__ list, int n, int c0,
                              int c1, int lane, F f) {
  for (int c = c0; c < c1; c += ALIGN_UNROLL) {
    int v[ALIGN_UNROLL];
#pragma unroll
    for (int u = 0; u < ALIGN_UNROLL; ++u) {
      const long i = (long)(c + u) * WAVE_SIZE + lane;
      v[u] = (c + u < c1 && i < n) ? list[i] : INT_MAX;
    }
#pragma unroll
    for (int u = 0; u < ALIGN_UNROLL; ++u)
      if (c + u < c1) f((c + u) * WAVE_SIZE, v[u]);
  }
}

__global__ void __launch_bounds__(ALIGN_WAVES* WAVE_SIZE)
moe_align_kernel(int* __restrict__ s_tok, int* __restrict__ order,
                 int* __restrict__ offs, int* __restrict__ counts,
                 const int* __restrict__ list, int n, int k) {
  __shared__ int s_lt[ALIGN_WAVES], s_eq[ALIGN_WAVES];
  const int e = blockIdx.x;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x >> 6;
  const int nchunks = (n + WAVE_SIZE - 1) / WAVE_SIZE;
  const int per_wave = (nchunks + ALIGN_WAVES - 1) / ALIGN_WAVES;
  const int c0 = min(wave * per_wave, nchunks);
  const int c1 = min(c0 + per_wave, nchunks);

  int lt = 0, eq = 0;
  for_chunks(list, n, c0, c1, lane, [&](int, int v) {
    lt += __popcll(__ballot(v < e));
    eq += __popcll(__ballot(v == e));
  });
  if (lane == 0) {
    s_lt[wave] = lt;
    s_eq[wave] = eq;
  }
  __syncthreads();
  int base = 0, total = 0;  // offs[e] + entries of e in earlier waves
#pragma unroll
  for (int w = 0; w < ALIGN_WAVES; ++w) {
    base += s_lt[w] + (w < wave ? s_eq[w] : 0);
    total += s_eq[w];
  }
  if (threadIdx.x == 0) {
    offs[e] = base;
    counts[e] = total;
  }
  if (eq == 0) return;

  const u64 below = ((u64)1 << lane) - 1;
  for_chunks(list, n, c0, c1, lane, [&](int first, int v) {
    const u64 m = __ballot(v == e);
    if (v == e) {
      const int pos = base + __popcll(m & below);
      order[pos] = first + lane;
      s_tok[pos] = (first + lane) / k;
    }
    base += __popcll(m);
  });
}

template <int VPL>
void route_launch(int* experts, float* weights, const float* logits,
                  const float* bias, int T, int E, int k, bool sigmoid,
                  bool renorm, int gshift, int n_group, int topk_group,
                  float scale, hipStream_t stream) {
  const dim3 grid(ceil_div(T, ROUTE_WAVES)), block(ROUTE_WAVES * WAVE_SIZE);
  if (sigmoid)
    moe_route_kernel<VPL, true><<<grid, block, 0, stream>>>(
        experts, weights, logits, bias, T, E, k, renorm, gshift, n_group,
        topk_group, scale);
  else
    moe_route_kernel<VPL, false><<<grid, block, 0, stream>>>(
        experts, weights, logits, bias, T, E, k, renorm, gshift, n_group,
        topk_group, scale);
}

}  // namespace

// *err = 1 for a shape outside the kernel's range (nothing is launched):
// 1 <= k <= min(16, E), E <= 512, n_group | E, group size 2..64 dividing 64,
// 1 <= topk_group <= n_group; groups only with the sigmoid router.
void moe_route_launch(int* experts, float* weights, const float* logits,
                      const float* bias, int T, int E, int k, int sigmoid,
                      int renorm, int n_group, int topk_group, float scale,
                      int* err, hipStream_t stream) {
  int gshift = 0;
  bool ok = T >= 1 && E >= 1 && E <= 512 && k >= 1 && k <= 16 && k <= E &&
            n_group >= 1 && E % n_group == 0 && topk_group >= 1 &&
            topk_group <= n_group;
  if (ok && n_group > 1) {
    const int gsz = E / n_group;
    while ((1 << gshift) < gsz) ++gshift;
    ok = sigmoid && gsz >= 2 && gsz <= WAVE_SIZE && (1 << gshift) == gsz;
  }
  *err = ok ? 0 : 1;
  if (!ok) return;
  const int vpl = ceil_div(E, WAVE_SIZE);
#define ROUTE_CASE(V)                                                       \
  route_launch<V>(experts, weights, logits, bias, T, E, k, sigmoid, renorm, \
                  gshift, n_group, topk_group, scale, stream)
  if (vpl <= 1) ROUTE_CASE(1);
  else if (vpl <= 2) ROUTE_CASE(2);
  else if (vpl <= 4) ROUTE_CASE(4);
  else if (vpl <= 6) ROUTE_CASE(6);
  else ROUTE_CASE(8);
#undef ROUTE_CASE
}

void moe_align_launch(int* s_tok, int* order, int* offs, int* counts,
                      const int* list, int n, int k, int E,
                      hipStream_t stream) {
  moe_align_kernel<<<dim3(E), dim3(ALIGN_WAVES * WAVE_SIZE), 0, stream>>>(
      s_tok, order, offs, counts, list, n, k);
}
