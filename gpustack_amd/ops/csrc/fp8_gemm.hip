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
// GEMM structure: the shared split-K tile of splitk_tile.h with the FP8
// element. BK = 128 fp8 elements keeps an LDS row at 128 B, so the staging
// and the swizzle are those of the bf16 skinny_gemm v1 byte for byte; why
// fragments are still read 16 B at a time is explained at the Fp8 policy.
#include "splitk_tile.h"

namespace {

using namespace splitk;

constexpr float F8_MAX = 448.f;

DEVICE_INLINE f32x4 f8_mfma(long a, long b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
}

// MI = 16-row fragments per wave along M; the block tile is (32*MI) x 128.
// MI=8 is the 256-row tile of the bf16 kernel; MI=2 (64 rows) serves small
// decode batches, where a 256-row X tile would triple the staging traffic.
template <int MI, bool WRITE_PARTIAL>
__global__ __launch_bounds__(THREADS) void fp8_gemm_kernel(
    void* __restrict__ out,            // bf16 [M,N] or f32 [S,M,N]
    const void* __restrict__ xq,       // [M, K] e4m3
    const float* __restrict__ xs,      // [M]
    const void* __restrict__ wq,       // [N, K] e4m3
    const float* __restrict__ ws,      // [N]
    int M, int N, int K, int splitk) {
  tile_body<Fp8, MI, WRITE_PARTIAL>(out, xq, xs, wq, ws, M, N, K, splitk);
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

}  // namespace

void fp8_gemm_launch(void* out, const void* xq, const void* xs,
                     const void* wq, const void* ws, void* workspace, int M,
                     int N, int K, int splitk, int* err_unsupported,
                     hipStream_t s) {
  constexpr int BK = ROW_BYTES / Fp8::ES;
  const bool ok = M >= 1 && N >= BN && N % BN == 0 && splitk >= 1 &&
                  splitk <= 16 && K >= BK * splitk &&
                  K % (BK * splitk) == 0 &&
                  (splitk == 1 || workspace != nullptr);
  *err_unsupported = !ok;
  if (!ok) return;
  if (M <= 64) {
    launch<64, BN, true>(fp8_gemm_kernel<2, true>, fp8_gemm_kernel<2, false>,
                         out, xq, (const float*)xs, wq, (const float*)ws,
                         workspace, M, N, K, splitk, s);
  } else {
    launch<256, BN, true>(fp8_gemm_kernel<8, true>, fp8_gemm_kernel<8, false>,
                          out, xq, (const float*)xs, wq, (const float*)ws,
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
