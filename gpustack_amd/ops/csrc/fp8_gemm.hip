// Dynamic W8A8 FP8 serving GEMM for MI355X (gfx950), OCP e4m3 (not fnuz).
//
//   out[m,n] = bf16( (sum_k xq[m,k] * wq[n,k]) * xs[m] * ws[n] )
//
// xq/wq are e4m3 codes, xs one f32 scale per token row, ws one f32 scale per
// output channel. Every fp8 x fp8 product is exact in f32, so the only
// freedom an implementation has is the order of the f32 sum.
//
// Kernels in this file:
//  - fp8_quant_rows: per-row amax -> scale = amax/448 -> clamp -> e4m3 codes
//  - fp8_gemm:       split-K MFMA GEMM on v_mfma_f32_16x16x32_fp8_fp8
//  - fp8_dequant:    exact e4m3 -> bf16 up-conversion (large-M fallback)
//  - fp8_mfma_probe: one wave, one instruction, checks the A/B lane map
//
// GEMM structure: the v1 kernel of skinny_gemm.hip with bytes for bf16.
// BK = 128 fp8 elements keeps an LDS row at 128 B, so the global_load_lds
// staging and the ((row&7)<<4) XOR swizzle carry over byte for byte.
//
// Fragment reads: the fp8 instruction takes 8 B of A and B per lane. Read as
// ds_read_b64 through the carried-over swizzle, the 32 lanes of a half-wave
// would touch 16 rows x 2 eight-byte halves; rows r and r+8 have equal
// (row&7) and equal parity, i.e. the same 16-B slot of the 256-B bank row,
// so that read is 2-way conflicted (the swizzle only separates 8 rows, which
// is all a 16-lane ds_read_b128 group needs). Instead each lane keeps the
// bf16 kernel's conflict-free ds_read_b128 and feeds its low and high 8 B to
// two consecutive MFMAs. That permutes k inside a 64-byte half-row (lane
// group g supplies bytes 16g..16g+7 to the first MFMA and 16g+8..16g+15 to
// the second), identically for A and B, so the dot product is unchanged and
// the kernel issues half the LDS reads.
#include "common.h"

namespace {

constexpr int F8_BN = 128;
constexpr int F8_BK = 128;             // fp8 elements == bytes per LDS row
constexpr int F8_WAVES = 8;
constexpr int F8_THREADS = F8_WAVES * WAVE_SIZE;
constexpr float F8_MAX = 448.f;

typedef __attribute__((ext_vector_type(2))) long i64x2;

DEVICE_INLINE f32x4 f8_mfma(long a, long b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
}

DEVICE_INLINE int f8_swz(int row, int colbyte) {
  return row * F8_BK + (colbyte ^ ((row & 7) << 4));
}

// MI = 16-row fragments per wave along M; the block tile is (32*MI) x 128.
// MI=8 is the 256-row tile of the bf16 kernel; MI=2 (64 rows) serves small
// decode batches, where a 256-row X tile would triple the staging traffic.
template <int MI, bool WRITE_PARTIAL>
__global__ __launch_bounds__(F8_THREADS) void fp8_gemm_kernel(
    void* __restrict__ out,                  // bf16 [M,N] or f32 [S,M,N]
    const unsigned char* __restrict__ xq,    // [M, K] e4m3
    const float* __restrict__ xs,            // [M]
    const unsigned char* __restrict__ wq,    // [N, K] e4m3
    const float* __restrict__ ws,            // [N]
    int M, int N, int K, int splitk) {
  constexpr int BM = 32 * MI;
  constexpr int XCHUNKS = BM * F8_BK / 16 / F8_THREADS;   // 16-B chunks/thread
  static_assert(XCHUNKS >= 1, "X tile must give every thread a chunk");
  const int mt = (M + BM - 1) / BM;
  int tid = blockIdx.x;
  const int split = tid % splitk;
  tid /= splitk;
  const int m0 = (tid % mt) * BM;
  const int n0 = (tid / mt) * F8_BN;
  const int kchunk = K / splitk;          // multiple of F8_BK (host-checked)
  const int k0 = split * kchunk;
  const int nk = kchunk / F8_BK;

  __shared__ unsigned char Xl[2][BM * F8_BK];
  __shared__ unsigned char Wl[2][F8_BN * F8_BK];

  const int t = threadIdx.x;
  const int lane = t & (WAVE_SIZE - 1);
  const int wid = t / WAVE_SIZE;
  const int wm = wid >> 2;                // 0..1  (row half)
  const int wn = wid & 3;                 // 0..3  (col quarter)
  const int lc = lane & 15;
  const int lg = lane >> 4;

  // linear LDS byte L of a 16-B chunk maps to logical (row = L/128,
  // colbyte = (L%128) ^ swz(row)); the global source reads that element.
  auto stage = [&](int buf, int kb) {
    const long kbase = k0 + (long)kb * F8_BK;
#pragma unroll
    for (int r = 0; r < XCHUNKS; ++r) {
      const int L = (t + r * F8_THREADS) * 16;
      const int row = L / F8_BK;
      const int colbyte = (L % F8_BK) ^ ((row & 7) << 4);
      int grow = m0 + row;
      if (grow >= M) grow = M - 1;        // clamp (masked at write)
      const unsigned char* src = xq + (long)grow * K + kbase + colbyte;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)(Xl[buf] + L),
          16, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int L = (t + r * F8_THREADS) * 16;
      const int row = L / F8_BK;
      const int colbyte = (L % F8_BK) ^ ((row & 7) << 4);
      const unsigned char* src = wq + (long)(n0 + row) * K + kbase + colbyte;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)(Wl[buf] + L),
          16, 0, 0);
    }
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
  for (int kb = 0; kb < nk; ++kb) {
    if (kb + 1 < nk) stage(buf ^ 1, kb + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {          // 64-byte half-row = 2 k-steps
      const int colbyte = h * 64 + lg * 16;
      i64x2 bfrag[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int row = wn * 32 + ni * 16 + lc;       // W row (output col)
        bfrag[ni] = *reinterpret_cast<const i64x2*>(
            Wl[buf] + f8_swz(row, colbyte));
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int row = wm * (16 * MI) + mi * 16 + lc;  // X row (output row)
        const i64x2 a = *reinterpret_cast<const i64x2*>(
            Xl[buf] + f8_swz(row, colbyte));
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          acc[mi][ni] = f8_mfma(a[0], bfrag[ni][0], acc[mi][ni]);
          acc[mi][ni] = f8_mfma(a[1], bfrag[ni][1], acc[mi][ni]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: D row = (l>>4)*4 + r, col = l&15 per 16x16 fragment. The
  // scales multiply the f32 sum before the single bf16 rounding; with
  // split-K the reduce kernel does that on the final sum instead.
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int gcol = n0 + wn * 32 + ni * 16 + lc;
    const float wsc = WRITE_PARTIAL ? 1.f : ws[gcol];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int grow = m0 + wm * (16 * MI) + mi * 16 + lg * 4 + r;
        if (grow >= M) continue;
        if (WRITE_PARTIAL) {
          reinterpret_cast<float*>(out)[((long)split * M + grow) * N + gcol] =
              acc[mi][ni][r];
        } else {
          reinterpret_cast<unsigned short*>(out)[(long)grow * N + gcol] =
              f2bf(acc[mi][ni][r] * xs[grow] * wsc);
        }
      }
    }
  }
}

// partial[S, M, N] f32 -> out[M, N] bf16; fixed summation order, no atomics
__global__ void fp8_reduce_kernel(unsigned short* __restrict__ out,
                                  const float* __restrict__ partial,
                                  const float* __restrict__ xs,
                                  const float* __restrict__ ws,
                                  long MN, int N, int splitk) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < MN;
       i += (long)gridDim.x * blockDim.x) {
    float a = 0.f;
    for (int s = 0; s < splitk; ++s) a += partial[s * MN + i];
    out[i] = f2bf(a * xs[i / N] * ws[i % N]);
  }
}

// ---------------------------------------------------------------------------
// Row quantization: one block per row. H <= 8192 keeps the row in registers
// (256 thr * 4 * u16x8); longer rows are re-read through L2.
// ---------------------------------------------------------------------------
constexpr int Q_THREADS = 256;
constexpr int Q_MAX_VEC = 4;

DEVICE_INLINE float q_amax8(const u16x8 u, float m) {
#pragma unroll
  for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(bf2f(u[i])));
  return m;
}

// clamp BEFORE the convert, true f32 division (no reciprocal) so the codes
// match the host definition bit for bit
DEVICE_INLINE void q_store8(unsigned char* dst, const u16x8 u, float scale) {
  float q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    q[i] = fminf(fmaxf(bf2f(u[i]) / scale, -F8_MAX), F8_MAX);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], hi, true);
  *reinterpret_cast<uint2*>(dst) = make_uint2((unsigned)lo, (unsigned)hi);
}

__global__ __launch_bounds__(Q_THREADS) void fp8_quant_rows_kernel(
    unsigned char* __restrict__ xq, float* __restrict__ xs,
    const unsigned short* __restrict__ x, int M, int K) {
  const int nvec = K / 8;  // K % 8 == 0 enforced on host
  const bool cached = nvec <= Q_THREADS * Q_MAX_VEC;
  __shared__ float red[Q_THREADS / WAVE_SIZE];
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const unsigned short* rp = x + (long)row * K;
    unsigned char* qp = xq + (long)row * K;
    u16x8 vals[Q_MAX_VEC];
    float amax = 0.f;
    if (cached) {
#pragma unroll
      for (int slot = 0; slot < Q_MAX_VEC; ++slot) {
        const int v = threadIdx.x + slot * Q_THREADS;
        if (v < nvec) {
          vals[slot] = *reinterpret_cast<const u16x8*>(rp + v * 8);
          amax = q_amax8(vals[slot], amax);
        }
      }
    } else {
      for (int v = threadIdx.x; v < nvec; v += Q_THREADS)
        amax = q_amax8(*reinterpret_cast<const u16x8*>(rp + v * 8), amax);
    }
    amax = wave_reduce_max(amax);
    if ((threadIdx.x & (WAVE_SIZE - 1)) == 0) red[threadIdx.x / WAVE_SIZE] = amax;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < Q_THREADS / WAVE_SIZE; ++i) tot = fmaxf(tot, red[i]);
    const float scale = tot > 0.f ? tot / F8_MAX : 1.f;
    if (threadIdx.x == 0) xs[row] = scale;
    if (cached) {
#pragma unroll
      for (int slot = 0; slot < Q_MAX_VEC; ++slot) {
        const int v = threadIdx.x + slot * Q_THREADS;
        if (v < nvec) q_store8(qp + v * 8, vals[slot], scale);
      }
    } else {
      for (int v = threadIdx.x; v < nvec; v += Q_THREADS)
        q_store8(qp + v * 8, *reinterpret_cast<const u16x8*>(rp + v * 8),
                 scale);
    }
    __syncthreads();
  }
}

// e4m3 -> bf16, exact (3 mantissa bits fit in 7; the exponent range fits)
__global__ void fp8_dequant_kernel(unsigned short* __restrict__ out,
                                   const unsigned char* __restrict__ q,
                                   long n) {
  const long nvec = n / 8;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
       v += (long)gridDim.x * blockDim.x) {
    const uint2 c = *reinterpret_cast<const uint2*>(q + v * 8);
    float f[8];
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
    const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false);
    const f32x2 e = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
    f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
    f[4] = d[0]; f[5] = d[1]; f[6] = e[0]; f[7] = e[1];
    *reinterpret_cast<u16x8*>(out + v * 8) = f32_to_bf8(f);
  }
  if (blockIdx.x == 0) {
    for (long i = nvec * 8 + threadIdx.x; i < n; i += blockDim.x)
      out[i] = f2bf(fp8_to_f32(q[i]));
  }
}

// fallback epilogue: out[m,n] = bf16(out[m,n] * xs[m] * ws[n]) in place
// (N % 8 == 0 enforced on host)
__global__ void fp8_scale_out_kernel(unsigned short* __restrict__ out,
                                     const float* __restrict__ xs,
                                     const float* __restrict__ ws,
                                     long MN, int N) {
  const long nvec = MN / 8;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
       v += (long)gridDim.x * blockDim.x) {
    const long i = v * 8;
    const float rs = xs[i / N];
    const int c = (int)(i % N);
    u16x8 u = *reinterpret_cast<const u16x8*>(out + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = f2bf(bf2f(u[j]) * rs * ws[c + j]);
    *reinterpret_cast<u16x8*>(out + i) = u;
  }
}

// D = A[16x32] * B[32x16], e4m3 in / f32 out. Assumed lane map (the bf16
// one with bytes): lane l holds A[l&15][8*(l>>4) + j] and
// B[8*(l>>4) + j][l&15] in byte j of its 64-bit operand.
__global__ void fp8_mfma_probe_kernel(float* __restrict__ d,
                                      const unsigned char* __restrict__ a,
                                      const unsigned char* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int lc = lane & 15, lg = lane >> 4;
  unsigned long af = 0, bf = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af |= (unsigned long)a[lc * 32 + lg * 8 + j] << (8 * j);
    bf |= (unsigned long)b[(lg * 8 + j) * 16 + lc] << (8 * j);
  }
  f32x4 c{0.f, 0.f, 0.f, 0.f};
  c = f8_mfma((long)af, (long)bf, c);
#pragma unroll
  for (int r = 0; r < 4; ++r) d[(lg * 4 + r) * 16 + lc] = c[r];
}

template <int MI>
void fp8_gemm_dispatch(void* out, const unsigned char* xq, const float* xs,
                       const unsigned char* wq, const float* ws,
                       void* workspace, int M, int N, int K, int splitk,
                       hipStream_t s) {
  constexpr int BM = 32 * MI;
  const int mt = (M + BM - 1) / BM;
  const int nt = N / F8_BN;
  dim3 grid(mt * nt * splitk);
  dim3 block(F8_THREADS);
  if (splitk > 1) {
    hipLaunchKernelGGL((fp8_gemm_kernel<MI, true>), grid, block, 0, s,
                       workspace, xq, xs, wq, ws, M, N, K, splitk);
    const long MN = (long)M * N;
    int rgrid = (int)((MN + 255) / 256);
    if (rgrid > 2048) rgrid = 2048;
    hipLaunchKernelGGL(fp8_reduce_kernel, dim3(rgrid), dim3(256), 0, s,
                       (unsigned short*)out, (const float*)workspace, xs, ws,
                       MN, N, splitk);
  } else {
    hipLaunchKernelGGL((fp8_gemm_kernel<MI, false>), grid, block, 0, s, out,
                       xq, xs, wq, ws, M, N, K, splitk);
  }
}

}  // namespace

void fp8_gemm_launch(void* out, const void* xq, const void* xs,
                     const void* wq, const void* ws, void* workspace, int M,
                     int N, int K, int splitk, int* err_unsupported,
                     hipStream_t s) {
  const bool ok = M >= 1 && N >= F8_BN && N % F8_BN == 0 && splitk >= 1 &&
                  splitk <= 16 && K >= F8_BK * splitk &&
                  K % (F8_BK * splitk) == 0 &&
                  (splitk == 1 || workspace != nullptr);
  *err_unsupported = !ok;
  if (!ok) return;
  if (M <= 64) {
    fp8_gemm_dispatch<2>(out, (const unsigned char*)xq, (const float*)xs,
                         (const unsigned char*)wq, (const float*)ws,
                         workspace, M, N, K, splitk, s);
  } else {
    fp8_gemm_dispatch<8>(out, (const unsigned char*)xq, (const float*)xs,
                         (const unsigned char*)wq, (const float*)ws,
                         workspace, M, N, K, splitk, s);
  }
}

void fp8_quant_rows_launch(void* xq, void* xs, const void* x, int M, int K,
                           int* err_unsupported, hipStream_t s) {
  const bool ok = M >= 1 && K >= 8 && K % 8 == 0;
  *err_unsupported = !ok;
  if (!ok) return;
  hipLaunchKernelGGL(fp8_quant_rows_kernel, dim3(M < 65535 ? M : 65535),
                     dim3(Q_THREADS), 0, s, (unsigned char*)xq, (float*)xs,
                     (const unsigned short*)x, M, K);
}

void fp8_dequant_launch(void* out, const void* q, long n, hipStream_t s) {
  if (n <= 0) return;
  long grid = (n / 8 + 255) / 256;
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(fp8_dequant_kernel, dim3((int)grid), dim3(256), 0, s,
                     (unsigned short*)out, (const unsigned char*)q, n);
}

void fp8_scale_out_launch(void* out, const void* xs, const void* ws, long M,
                          int N, int* err_unsupported, hipStream_t s) {
  const bool ok = M >= 1 && N >= 8 && N % 8 == 0;
  *err_unsupported = !ok;
  if (!ok) return;
  const long MN = M * N;
  long grid = (MN / 8 + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(fp8_scale_out_kernel, dim3((int)grid), dim3(256), 0, s,
                     (unsigned short*)out, (const float*)xs, (const float*)ws,
                     MN, N);
}

void fp8_mfma_probe_launch(float* d, const void* a, const void* b,
                           hipStream_t s) {
  hipLaunchKernelGGL(fp8_mfma_probe_kernel, dim3(1), dim3(64), 0, s, d,
                     (const unsigned char*)a, (const unsigned char*)b);
}
