// Fused top-k / top-p / min-p sampling for MI355X (gfx950).
//
// One 256-thread block draws one token for one row of bf16 logits from that
// row's own (temperature, top_k, top_p, min_p, seed, step). There is no sort:
// bf16 has 65,536 distinct values, so under a monotone 16-bit key the exact
// top-k and nucleus thresholds come out of a two-level radix select in LDS
// (4096 bins on the top 12 key bits, then the 16 keys of the crossing bin).
//
// Every sum that decides a result is an integer sum, so the result does not
// depend on the order of adds: a token's weight w = exp((l - max)/T) is
// turned into the fixed-point value floor(w * 2^32) once, and masses are u64
// sums of those. A row's result depends on that row's inputs alone.
//
// Passes over the row (it stays in L2 between them):
//   A  max + argmax (greedy rows stop here)
//   B  level-1 histogram: count and mass per 12-bit bin
//   C  level-2 histogram: counts of the 16 keys of the two crossing bins
//   D  kept mass per thread (each thread owns a contiguous chunk of the row)
//   E  one wave walks the chunk that holds the draw, in index order
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / WAVE_SIZE;
constexpr int L2_BITS = 4;
constexpr int L1_BINS = 1 << (16 - L2_BITS);
constexpr int L2_BINS = 1 << L2_BITS;
constexpr int BINS_PER_THREAD = L1_BINS / SAMPLE_THREADS;

// bf16 bits -> 16-bit key with the order of the float values (-0 == +0).
DEVICE_INLINE unsigned key16(unsigned short u) {
  unsigned x = u;
  if (x == 0x8000u) x = 0;
  return (x & 0x8000u) ? (~x & 0xffffu) : (x | 0x8000u);
}

DEVICE_INLINE unsigned short unkey16(unsigned k) {
  return (unsigned short)((k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu));
}

// w = exp((l - M)/T) as 2^((l - M) * log2(e)/T) on the hardware exp2, in
// [0, 1]; anything else (NaN from inf - inf) counts as 0. The passes are
// bound by their arithmetic per element, and the library expf costs more
// than everything else in them together.
DEVICE_INLINE float weight(unsigned short bits, float M, float scale) {
  const float w = __builtin_amdgcn_exp2f((bf2f(bits) - M) * scale);
  return fminf(fmaxf(w, 0.f), 1.f);
}

DEVICE_INLINE u64 fix32(float w) { return (u64)(w * 4294967296.0f); }

// Eight consecutive elements of the row. Vector slot vv covers the real
// indices [8*vv - a, 8*vv - a + 8), where a is the row's offset (in
// elements) from a 16-byte boundary, so that a full slot is an aligned
// 16-byte load; the partial slots at both ends load element by element.
// Returns the mask of elements that lie inside [0, V).
DEVICE_INLINE unsigned load8(const unsigned short* __restrict__ rp, int a,
                             int V, int vv, u16x8& out) {
  const int i0 = vv * 8 - a;
  if (i0 >= 0 && i0 + 8 <= V) {
    out = *reinterpret_cast<const u16x8*>(rp + i0);
    return 0xffu;
  }
  unsigned mask = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = i0 + j;
    unsigned short x = 0;
    if (i >= 0 && i < V) {
      x = rp[i];
      mask |= 1u << j;
    }
    out[j] = x;
  }
  return mask;
}

// Calls f(vv, u, mask) for the slots first, first + stride, ... below end.
// The row is read from L2 by one block, so latency bounds every pass: full
// slots are loaded four at a time ahead of their use.
template <class F>
DEVICE_INLINE void for_slots(const unsigned short* __restrict__ rp, int a,
                             int V, int first, int stride, int end, F f) {
  const int full_lo = a ? 1 : 0;  // slots [full_lo, full_hi) are full
  int full_hi = (V + a) / 8;
  if (full_hi > end) full_hi = end;
  int vv = first;
  if (vv < full_lo && vv < end) {  // the partial head slot
    u16x8 u;
    const unsigned mask = load8(rp, a, V, vv, u);
    f(vv, u, mask);
    vv += stride;
  }
  for (; vv + 3 * stride < full_hi; vv += 4 * stride) {
    u16x8 u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      u[q] = *reinterpret_cast<const u16x8*>(rp + (vv + q * stride) * 8 - a);
#pragma unroll
    for (int q = 0; q < 4; ++q) f(vv + q * stride, u[q], 0xffu);
  }
  for (; vv < end; vv += stride) {
    u16x8 u;
    const unsigned mask = load8(rp, a, V, vv, u);
    f(vv, u, mask);
  }
}

// First output word of Philox4x32-10, key = seed, counter = (step, 0, 0).
DEVICE_INLINE unsigned philox_x0(u64 seed, u64 step) {
  unsigned c0 = (unsigned)step, c1 = (unsigned)(step >> 32), c2 = 0, c3 = 0;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// Sum of v over the threads above this one (above) and over the block
// (total). red: SAMPLE_WAVES words of LDS, free again on return.
DEVICE_INLINE void block_suffix_sum(u64 v, u64* red, u64& above, u64& total) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x / WAVE_SIZE;
  u64 incl = v;
#pragma unroll
  for (int d = 1; d < WAVE_SIZE; d <<= 1) {
    const u64 t = __shfl_down(incl, d, WAVE_SIZE);
    if (lane + d < WAVE_SIZE) incl += t;
  }
  if (lane == 0) red[wid] = incl;
  __syncthreads();
  above = incl - v;
  total = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) {
    const u64 s = red[w];
    total += s;
    if (w > wid) above += s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(
    long* __restrict__ out, const unsigned short* __restrict__ logits,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ min_p,
    const long* __restrict__ seed, const long* __restrict__ step, int N,
    int V) {
  const int row = blockIdx.x;
  if (row >= N) return;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wid = tid / WAVE_SIZE;
  const unsigned short* rp = logits + (long)row * V;
  const int a = (int)((reinterpret_cast<uintptr_t>(rp) >> 1) & 7);
  const int NV = (V + a + 7) / 8;

  __shared__ unsigned s_cnt[L1_BINS];
  __shared__ u64 s_mass[L1_BINS];
  __shared__ u64 s_red[SAMPLE_WAVES];
  __shared__ float s_bv[SAMPLE_WAVES];
  __shared__ int s_bi[SAMPLE_WAVES];
  __shared__ unsigned s_ck[L2_BINS], s_cp[L2_BINS];
  __shared__ int s_bk, s_bp;
  __shared__ u64 s_cabove, s_pabove;
  __shared__ unsigned s_tau_k, s_tau_p;
  __shared__ int s_owner;
  __shared__ u64 s_before;

  // ---- pass A: max and argmax (ties -> lowest index) ----------------------
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for_slots(rp, a, V, tid, SAMPLE_THREADS, NV,
            [&](int vv, const u16x8& u, unsigned mask) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!(mask >> j & 1u)) continue;
      const float f = bf2f(u[j]);
      const int gi = vv * 8 - a + j;
      if (f > best || (f == best && gi < besti)) { best = f; besti = gi; }
    }
  });
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(best, m, WAVE_SIZE);
    const int oi = __shfl_xor(besti, m, WAVE_SIZE);
    if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
  }
  if (lane == 0) { s_bv[wid] = best; s_bi[wid] = besti; }
  __syncthreads();
  best = s_bv[0]; besti = s_bi[0];
#pragma unroll
  for (int w = 1; w < SAMPLE_WAVES; ++w) {
    if (s_bv[w] > best || (s_bv[w] == best && s_bi[w] < besti)) {
      best = s_bv[w]; besti = s_bi[w];
    }
  }
  // the answer of a greedy row, and of any row whose weights all vanish
  const int amax = besti < V ? besti : 0;
  if (tid == 0) out[row] = amax;
  const float T = temperature[row];
  if (!(T > 0.f)) return;

  const float M = best;
  const float w_scale = 1.4426950408889634f / T;  // log2(e)/T
  const unsigned key_max = key16((unsigned short)(__float_as_uint(M) >> 16));
  const int k = top_k[row];
  const float p = top_p[row];
  const float mp = min_p[row];
  const bool k_on = k > 0 && k < V;
  const bool p_on = p < 1.f;
  const bool mp_on = mp > 0.f;

  unsigned tau = 0;
  if (k_on || p_on) {
    // ---- pass B: level-1 histogram ----------------------------------------
    for (int b = tid; b < L1_BINS; b += SAMPLE_THREADS) {
      s_cnt[b] = 0;
      s_mass[b] = 0;
    }
    if (tid < L2_BINS) { s_ck[tid] = 0; s_cp[tid] = 0; }
    if (tid == 0) {
      s_bk = 0; s_cabove = 0; s_tau_k = 0;
      s_bp = L1_BINS - 1; s_pabove = 0; s_tau_p = p_on ? key_max : 0;
    }
    __syncthreads();
    for_slots(rp, a, V, tid, SAMPLE_THREADS, NV,
              [&](int, const u16x8& u, unsigned mask) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!(mask >> j & 1u)) continue;
        const unsigned bin = key16(u[j]) >> L2_BITS;
        atomicAdd(&s_cnt[bin], 1u);
        const u64 wf = fix32(weight(u[j], M, w_scale));
        if (wf) atomicAdd(&s_mass[bin], wf);
      }
    });
    __syncthreads();

    // ---- level-1 select: thread t owns bins [16t, 16t + 16) ---------------
    const int lo = tid * BINS_PER_THREAD;
    u64 lc = 0, lm = 0;
#pragma unroll
    for (int b = 0; b < BINS_PER_THREAD; ++b) {
      lc += s_cnt[lo + b];
      lm += s_mass[lo + b];
    }
    u64 c_above, c_total, m_above, Z;
    block_suffix_sum(lc, s_red, c_above, c_total);
    block_suffix_sum(lm, s_red, m_above, Z);
    const double pz = (double)p * (double)Z;
    if (k_on) {
      // the bin in which the count of tokens at or above reaches k
      u64 c = c_above;
      for (int b = lo + BINS_PER_THREAD - 1; b >= lo; --b) {
        const u64 c2 = c + s_cnt[b];
        if (c < (u64)k && c2 >= (u64)k) { s_bk = b; s_cabove = c; }
        c = c2;
      }
    }
    if (p_on) {
      // the lowest bin whose mass strictly above is still <= p*Z
      u64 m = m_above;
      for (int b = lo + BINS_PER_THREAD - 1; b >= lo; --b) {
        const u64 m2 = m + s_mass[b];
        if ((double)m <= pz && ((double)m2 > pz || b == 0)) {
          s_bp = b; s_pabove = m;
        }
        m = m2;
      }
    }
    __syncthreads();

    // ---- pass C: level-2 histogram of the crossing bins -------------------
    const unsigned bk = (unsigned)s_bk, bp = (unsigned)s_bp;
    for_slots(rp, a, V, tid, SAMPLE_THREADS, NV,
              [&](int, const u16x8& u, unsigned mask) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!(mask >> j & 1u)) continue;
        const unsigned key = key16(u[j]);
        const unsigned bin = key >> L2_BITS, sub = key & (L2_BINS - 1);
        if (k_on && bin == bk) atomicAdd(&s_ck[sub], 1u);
        if (p_on && bin == bp) atomicAdd(&s_cp[sub], 1u);
      }
    });
    __syncthreads();
    if (tid == 0) {
      if (k_on) {
        u64 c = s_cabove;
        for (int s = L2_BINS - 1; s >= 0; --s) {
          c += s_ck[s];
          if (c >= (u64)k) { s_tau_k = (bk << L2_BITS) | (unsigned)s; break; }
        }
      }
      if (p_on) {
        // a key's mass is its count times its weight: every token of that
        // key added the same fixed-point weight in pass B
        u64 m = s_pabove;
        for (int s = L2_BINS - 1; s >= 0; --s) {
          if (!((double)m <= pz)) break;
          const unsigned key = (bp << L2_BITS) | (unsigned)s;
          s_tau_p = key;
          m += (u64)s_cp[s] * fix32(weight(unkey16(key), M, w_scale));
        }
      }
    }
    __syncthreads();
    tau = s_tau_k > s_tau_p ? s_tau_k : s_tau_p;
  }

  // ---- pass D: kept mass, thread t owning slots [t*C, (t+1)*C) ------------
  const int C = (NV + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
  const int c_begin = tid * C;
  const int c_end = c_begin + C < NV ? c_begin + C : NV;
  u64 acc = 0;
  for_slots(rp, a, V, c_begin, 1, c_end,
            [&](int, const u16x8& u, unsigned mask) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!(mask >> j & 1u) || key16(u[j]) < tau) continue;
      const float w = weight(u[j], M, w_scale);
      if (!mp_on || w >= mp) acc += fix32(w);
    }
  });
  u64 above, S;
  block_suffix_sum(acc, s_red, above, S);
  if (S == 0) return;  // nothing drawable: the argmax stands
  const u64 before = S - above - acc;

  // target = floor(u * S) with u = m / 2^24, exact in 64 bits (S <= 2^63)
  const u64 m24 = philox_x0((u64)seed[row], (u64)step[row]) >> 8;
  const u64 target = m24 * (S >> 24) + ((m24 * (S & 0xffffffull)) >> 24);
  // the drawn token is the first kept one whose running mass exceeds
  // target; target < S, so exactly one thread's chunk holds it
  if (before <= target && target < before + acc) {
    s_owner = tid;
    s_before = before;
  }
  __syncthreads();
  if (wid != 0) return;

  // ---- pass E: wave 0 walks that chunk in index order ---------------------
  const int v_begin = s_owner * C;
  const int v_end = v_begin + C < NV ? v_begin + C : NV;
  u64 run = s_before;
  u16x8 u_next;
  unsigned mask_next =
      v_begin + lane < v_end ? load8(rp, a, V, v_begin + lane, u_next) : 0;
  for (int v0 = v_begin; v0 < v_end; v0 += WAVE_SIZE) {
    const int vv = v0 + lane;
    const u16x8 u = u_next;
    const unsigned mask = mask_next;
    // the next step's slot is on its way while this one is scanned
    mask_next = vv + WAVE_SIZE < v_end
                    ? load8(rp, a, V, vv + WAVE_SIZE, u_next) : 0;
    u64 e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      e[j] = 0;
      if (!(mask >> j & 1u) || key16(u[j]) < tau) continue;
      const float w = weight(u[j], M, w_scale);
      if (!mp_on || w >= mp) e[j] = fix32(w);
    }
    u64 ls = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) ls += e[j];
    u64 incl = ls;
#pragma unroll
    for (int d = 1; d < WAVE_SIZE; d <<= 1) {
      const u64 t = __shfl_up(incl, d, WAVE_SIZE);
      if (lane >= d) incl += t;
    }
    const u64 tot = __shfl(incl, WAVE_SIZE - 1, WAVE_SIZE);
    if (run + tot > target) {
      u64 c = run + incl - ls;
      if (c <= target && target < c + ls) {
        int pick = 0;
#pragma unroll
        for (int j = 7; j >= 0; --j) {
          // prefix through element j, highest j first: the last one that
          // still exceeds target is the first in index order
          u64 pj = c;
#pragma unroll
          for (int q = 0; q <= j; ++q) pj += e[q];
          if (pj > target) pick = j;
        }
        out[row] = vv * 8 - a + pick;
      }
      return;
    }
    run += tot;
  }
}

}  // namespace

void sample_launch(long* out, const void* logits, const float* temperature,
                   const int* top_k, const float* top_p, const float* min_p,
                   const long* seed, const long* step, int N, int V,
                   hipStream_t s) {
  if (N < 1) return;
  hipLaunchKernelGGL(sample_kernel, dim3(N), dim3(SAMPLE_THREADS), 0, s, out,
                     (const unsigned short*)logits, temperature, top_k, top_p,
                     min_p, seed, step, N, V);
}
