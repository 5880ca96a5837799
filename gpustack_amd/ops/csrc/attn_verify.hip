// Speculative-verify paged attention for MI355X (gfx950) on MFMA.
//
// A verify step feeds W = 1 + num_draft_tokens consecutive rows per sequence.
// The W rows of a sequence and the GQ query heads of one KV head attend to the
// same page stream, so the unit of work is the window: W*GQ query rows against
// one KV head's pages, each KV byte read once per window instead of once per
// row as the flattened decode kernel does.
//
//  - one workgroup per (group of W rows, kv head), 4 waves; wave w takes pages
//    w, w+4, ... up to the group's longest row and keeps its own online-softmax
//    state; the waves merge once at the end through LDS.
//  - tile row j*GQ + g is window row j, query head h*GQ + g; MT 16-row tiles
//    cover the W*GQ <= 64 rows, rows past W*GQ (or past N) are dead: zero q,
//    length 0, never stored.
//  - scores S^T = K . Q^T per page with mfma_f32_16x16x32_bf16: A = the page's
//    16 tokens x 128 dims as 16 B row loads straight from the pool, B = the Q
//    fragments, loaded once and resident (4 k-steps x 8 bf16 per lane and
//    tile). q keeps its bits; the softmax scale is applied to the f32 scores.
//    A lane ends up with one query row (lane%16) and four consecutive tokens
//    (4*(lane/16)+r), so a row max is two cross-lane steps (xor 16, 32) and
//    the row's denominator is summed per lane and reduced once after the loop.
//  - that score layout is the B operand of mfma_f32_16x16x16bf16_1k
//    (k = 4*(lane/16)+r, n = lane%16): O^T = V^T . P^T takes P rounded to bf16
//    once, with no shuffle. V^T needs four tokens of one head dim per lane:
//    the V page goes through a per-wave LDS buffer (16 B stores, rows padded
//    by 32 B) and comes back with the LDS transpose read ds_read_b64_tr_b16.
//    The output tile O^T[d][row] has the lane's own query row as its column,
//    so the softmax correction is a per-lane scalar.
//  - the block-table entry is fetched two pages ahead and the next page's K/V
//    loads are issued before the current page's MFMAs.
//  - the length mask is a compare against the lane's row length, applied only
//    to pages that reach past the group's shortest row.
//  - no atomics, no host sync, fixed grid: captures into the decode hipGraph.
//
// KV pool layout: [num_blocks, Hkv, 16, 128] bf16.
#include "common.h"

namespace {

constexpr int VF_BS = 16;        // tokens per KV block (page)
constexpr int VF_D = 128;        // head dim
constexpr int VF_WAVES = 4;
constexpr int VF_THREADS = VF_WAVES * WAVE_SIZE;
// staged V row in bf16 elements: 256 B + 32 B, so the 8 rows that one half
// of the wave reads in a transpose read start 8 banks apart
constexpr int VF_VROW = VF_D + 16;
// merge row in floats: +4 spreads the 16 rows of a b128 store over the banks
constexpr int VF_OROW = VF_D + 4;
constexpr float VF_LOG2E = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(8))) short vf_s16x8;
typedef __attribute__((ext_vector_type(4))) short vf_s16x4;
typedef __attribute__((address_space(3))) vf_s16x4 vf_lds_s16x4;

DEVICE_INLINE f32x4 vf_mfma_k32(u16x8 a, u16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(vf_s16x8, a), __builtin_bit_cast(vf_s16x8, b), c, 0, 0,
      0);
}

DEVICE_INLINE f32x4 vf_mfma_k16(vf_s16x4 a, vf_s16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

// The 16 lanes of a row of lanes address a 4 x 16 tile of b16, lane i the
// four elements [i/4][4*(i%4) .. +3]; lane i gets column i, rows 0..3.
DEVICE_INLINE vf_s16x4 vf_lds_read_tr(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((vf_lds_s16x4*)p);
}

template <int MT>
constexpr int vf_lds_bytes() {
  // merge buffers: acc [waves][MT*16][OROW] f32, then m and l [waves][MT*16];
  // the per-wave V staging (waves * 16 * VROW bf16) aliases their start
  return VF_WAVES * MT * 16 * (VF_OROW + 2) * 4;
}

// Waves per SIMD asked for: what the merge buffers leave room for (4, 2 and 1
// workgroups per CU); each instantiation fits its registers without scratch.
template <int MT>
__global__ __launch_bounds__(VF_THREADS, MT == 1 ? 4 : (MT == 2 ? 2 : 1))
void paged_attn_verify_kernel(
    unsigned short* __restrict__ out,        // [N, Hq, 128]
    const unsigned short* __restrict__ q,    // [N, Hq, 128], row stride q_stride
    const unsigned short* __restrict__ kc,   // [B, Hkv, 16, 128] bf16
    const unsigned short* __restrict__ vc,
    const int* __restrict__ block_tables,    // [N, max_blocks]
    const int* __restrict__ seq_lens,        // [N]
    int N, int W, int GQ, int Hkv, int max_blocks, float scale, long q_stride) {
  constexpr int D = VF_D, BS = VF_BS;
  static_assert(VF_WAVES * BS * VF_VROW * 2 <= vf_lds_bytes<MT>(),
                "V staging must fit under the merge buffers it aliases");
  __shared__ __attribute__((aligned(16))) float smem[vf_lds_bytes<MT>() / 4];

  const int grp = blockIdx.x;
  const int h = blockIdx.y;          // kv head
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int li = lane & 15;          // query row within a tile / K token
  const int lg = lane >> 4;          // token quad / 8-dim slice of a k-step
  const int row0 = grp * W;
  const int live = min(W, N - row0);  // rows of this group that exist
  const int nrows = W * GQ;           // tile rows in use

  int maxlen = 0, minlen = 0x7fffffff;
  for (int j = 0; j < live; ++j) {
    const int L = seq_lens[row0 + j];
    maxlen = max(maxlen, L);
    minlen = min(minlen, L);
  }
  // the group's table covers maxlen by contract; never index past its row
  const int npages = min((maxlen + BS - 1) / BS, max_blocks);
  const int full_pages = minlen / BS;  // pages every live row sees whole

  // Q fragments (B operand: k = dim, n = query row) and row lengths
  u16x8 qf[MT][4];
  int lenr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int R = t * 16 + li;
    const int j = R / GQ;
    const int g = R - j * GQ;
    const bool ok = R < nrows && j < live;
    // a dead row reads the group's first row (always there) and drops it:
    // no address past row N-1 is ever formed
    const long row = row0 + (ok ? j : 0);
    const int len = seq_lens[row];
    lenr[t] = ok ? len : 0;
    const unsigned short* qp =
        q + row * q_stride + ((long)h * GQ + (ok ? g : 0)) * D + lg * 8;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const u16x8 qv = *reinterpret_cast<const u16x8*>(qp + kk * 32);
      qf[t][kk] = ok ? qv : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  float m[MT], l[MT];       // running max (log2 domain), lane's share of sum
  f32x4 acc[MT][D / 16];    // O^T[d = dt*16 + 4*lg + r][row = li]
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) acc[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  unsigned short* vl =
      reinterpret_cast<unsigned short*>(smem) + wave * BS * VF_VROW;
  const int* bt = block_tables + (long)row0 * max_blocks;
  const float sl2 = scale * VF_LOG2E;

  struct Stage {
    u16x8 k[4], v[4];
  };
  auto issue = [&](Stage& st, int blk) {
    const long base = (((long)blk * Hkv + h) * BS) * D;
    const unsigned short* kp = kc + base + li * D + lg * 8;   // token li
    const unsigned short* vp = vc + base + lg * D + li * 8;   // tokens lg + 4*it
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      st.k[kk] = *reinterpret_cast<const u16x8*>(kp + kk * 32);
#pragma unroll
    for (int it = 0; it < 4; ++it)
      st.v[it] = *reinterpret_cast<const u16x8*>(vp + it * 4 * D);
  };

  int page = wave;
  int blk_next = 0;
  Stage cur;
  if (page < npages) {
    issue(cur, bt[page]);
    if (page + VF_WAVES < npages) blk_next = bt[page + VF_WAVES];
  }
  while (page < npages) {
    const bool more = page + VF_WAVES < npages;
    // stage this page's V: token lg + 4*it, dims [8*li, 8*li + 8)
#pragma unroll
    for (int it = 0; it < 4; ++it)
      *reinterpret_cast<u16x8*>(vl + (it * 4 + lg) * VF_VROW + li * 8) =
          cur.v[it];
    Stage nxt;
    int blk_next2 = 0;
    if (more) {
      issue(nxt, blk_next);
      if (page + 2 * VF_WAVES < npages) blk_next2 = bt[page + 2 * VF_WAVES];
    }
    // the staged page is read back by other lanes of this wave
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    const bool partial = page >= full_pages;
    const int tok0 = page * BS + lg * 4;
    vf_s16x4 pb[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = vf_mfma_k32(cur.k[kk], qf[t][kk], s);
      float x[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = s[r] * sl2;
      if (partial) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          x[r] = (tok0 + r < lenr[t]) ? x[r] : -INFINITY;
      }
      float pm = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
      pm = fmaxf(pm, __shfl_xor(pm, 16, WAVE_SIZE));
      pm = fmaxf(pm, __shfl_xor(pm, 32, WAVE_SIZE));
      const float nm = fmaxf(m[t], pm);
      // a row that has seen no key yet keeps m = -inf, p = 0, corr = 0
      const float ref = (nm == -INFINITY) ? 0.f : nm;
      const float corr = __builtin_amdgcn_exp2f(m[t] - ref);
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(x[r] - ref);
      l[t] = l[t] * corr + ((p[0] + p[1]) + (p[2] + p[3]));
      m[t] = nm;
      const u16x4 pu = {f2bf(p[0]), f2bf(p[1]), f2bf(p[2]), f2bf(p[3])};
      pb[t] = __builtin_bit_cast(vf_s16x4, pu);
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) acc[t][dt] *= corr;
    }

    // V^T fragments: lane needs V[4*lg + r][dt*16 + li], r = 0..3
    const unsigned short* vr = vl + (lg * 4 + (li >> 2)) * VF_VROW + (li & 3) * 4;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      const vf_s16x4 vt = vf_lds_read_tr(vr + dt * 16);
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t][dt] = vf_mfma_k16(vt, pb[t], acc[t][dt]);
    }
    // the next page's stores must stay behind these reads
    asm volatile("" ::: "memory");

    if (more) cur = nxt;
    blk_next = blk_next2;
    page += VF_WAVES;
  }

  // lane groups hold disjoint token quads of the same rows: sum their shares
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    l[t] += __shfl_xor(l[t], 16, WAVE_SIZE);
    l[t] += __shfl_xor(l[t], 32, WAVE_SIZE);
  }

  // Cross-wave merge through LDS (over the staging buffers, once every wave
  // has left the page loop).
  float* lds_acc = smem;                                   // [waves][MT*16][OROW]
  float* lds_m = smem + VF_WAVES * MT * 16 * VF_OROW;      // [waves][MT*16]
  float* lds_l = lds_m + VF_WAVES * MT * 16;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int R = t * 16 + li;
    float* arow = lds_acc + ((long)wave * MT * 16 + R) * VF_OROW + lg * 4;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      *reinterpret_cast<f32x4*>(arow + dt * 16) = acc[t][dt];
    if (lg == 0) {
      lds_m[wave * MT * 16 + R] = m[t];
      lds_l[wave * MT * 16 + R] = l[t];
    }
  }
  __syncthreads();

  const int Hq = Hkv * GQ;
  for (int u = threadIdx.x; u < nrows * D; u += VF_THREADS) {
    const int R = u / D;
    const int d = u % D;
    const int j = R / GQ;
    const int g = R - j * GQ;
    if (j >= live) break;  // rows past N: not stored (R only grows with u)
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < VF_WAVES; ++w)
      if (lds_l[w * MT * 16 + R] > 0.f) M = fmaxf(M, lds_m[w * MT * 16 + R]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < VF_WAVES; ++w) {
      const float lw = lds_l[w * MT * 16 + R];
      if (lw > 0.f) {
        const float wt = __builtin_amdgcn_exp2f(lds_m[w * MT * 16 + R] - M);
        num += wt * lds_acc[((long)w * MT * 16 + R) * VF_OROW + d];
        den += wt * lw;
      }
    }
    out[((long)(row0 + j) * Hq + (long)h * GQ + g) * D + d] =
        f2bf(den > 0.f ? num / den : 0.f);
  }
}

}  // namespace

void paged_attn_verify_launch(void* out, const void* q, const void* kc,
                              const void* vc, const int* block_tables,
                              const int* seq_lens, int N, int Hq, int Hkv,
                              int W, int max_blocks, float scale, long q_stride,
                              int* err_unsupported, hipStream_t s) {
  *err_unsupported = 0;
  const int GQ = Hkv > 0 ? Hq / Hkv : 0;
  if (GQ < 1 || GQ * Hkv != Hq || W < 2 || W > 8 || W * GQ > 64) {
    *err_unsupported = 1;
    return;
  }
  if (N <= 0) return;
  dim3 grid(ceil_div(N, W), Hkv);
  dim3 block(VF_THREADS);
  const int mt = ceil_div(W * GQ, 16);
#define LAUNCH_VERIFY(MT)                                                      \
  hipLaunchKernelGGL((paged_attn_verify_kernel<MT>), grid, block, 0, s,        \
                     (unsigned short*)out, (const unsigned short*)q,           \
                     (const unsigned short*)kc, (const unsigned short*)vc,     \
                     block_tables, seq_lens, N, W, GQ, Hkv, max_blocks, scale, \
                     q_stride)
  if (mt == 1) LAUNCH_VERIFY(1);
  else if (mt == 2) LAUNCH_VERIFY(2);
  else LAUNCH_VERIFY(4);
#undef LAUNCH_VERIFY
}
