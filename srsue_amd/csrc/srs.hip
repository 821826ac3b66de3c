// srs.hip -- the sounding reference signal on gfx950 (36.211 5.5.3.1, 5.5.3.2, 5.6; normal CP).
//
//   srs_kernel   grid (transmission, 1 + SRS_ZERO_PARTS).  Workgroup y = 0 makes SC-FDMA symbol 13.  The SRS sits on
//                every second subcarrier, a_{k0 + 2 k'} = r(k'), so with K = k0 - 6 N_RB
//                  s(n) = exp(j pi (2 K + 1) n / N) / sqrt(N) . sum_k' r(k') exp(j 2 pi k' n / (N / 2)),
//                and the sum has period N / 2: one N / 2 point inverse Stockham transform (64 .. 1024 points, radices
//                3, 4, 2; at most one butterfly per lane and pass, so the passes run in place in 8 KiB of LDS with
//                twiddles from sincospif on exact integer arguments) instead of an N point one.  The sequence is
//                generated straight into LDS: r(k') = exp(j 2 pi n_cs k' / 8) x_q(k' mod N_ZC), the Zadoff-Chu phase
//                q m (m + 1) mod 2 N_ZC reduced in 64-bit integers, or the tabulated M_sc = 24 sequence.  Then the
//                N + CP output samples read lds[n mod N / 2] times the phase factor; the tail (half-subcarrier
//                shift, cyclic prefix, scale, cfo) is that of pucch_kernel.  Workgroups y = 1 .. write the zeros of
//                symbols 0..12 (absent with MI_SRS_FLAG_LAST_SYMBOL_ONLY).
#include <hip/hip_runtime.h>

#include "srs.h"
#include "ul_seq_dev.h"

namespace mi {

namespace {

// unnormalised inverse DFT of 2 points in registers (exp(+j ...)), beside the shared 3- and 4-point ones
using mi::idft;
__device__ __forceinline__ void idft(float2 (&v)[2]) {
  const float2 a = v[0];
  v[0] = cadd(a, v[1]);
  v[1] = csub(a, v[1]);
}

// one Stockham pass of radix R over the H points of buf, in place, NS = the product of the earlier radices:
// butterfly j < H / R <= SRS_THREADS (one per lane) reads buf[j + r H / R], twiddles by exp(j 2 pi r (j mod NS) /
// (NS R)) and, once every lane has read, writes buf[(j / NS) NS R + j mod NS + r NS].  Ends with a barrier.
template <uint32_t R>
__device__ __forceinline__ void pass(float2* __restrict__ buf, uint32_t H, uint32_t NS, uint32_t t) {
  const uint32_t NB = H / R, k = t % NS;
  const bool on = t < NB;
  float2 v[R];
  if (on) {
#pragma unroll
    for (uint32_t r = 0; r < R; r++) v[r] = buf[t + r * NB];
    if (NS > 1) {
      const float step = 2.0f / (float)(NS * R);
#pragma unroll
      for (uint32_t r = 1; r < R; r++) {
        float s, c;
        sincospif((float)(r * k) * step, &s, &c);   // r k < 3 NS: exact in float
        v[r] = cmul(v[r], make_float2(c, s));
      }
    }
    idft(v);
  }
  __syncthreads();
  if (on) {
    const uint32_t j0 = (t / NS) * (NS * R) + k;
#pragma unroll
    for (uint32_t r = 0; r < R; r++) buf[j0 + r * NS] = v[r];
  }
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(SRS_THREADS) void srs_kernel(const MiSrsTx* __restrict__ txs,
                                                          const float* __restrict__ cfo,
                                                          const float* __restrict__ scale,
                                                          float2* __restrict__ iq) {
  __shared__ float2 buf[SRS_HMAX];
  const MiSrsTx x = txs[blockIdx.x];
  const uint32_t t = threadIdx.x, N = x.N, H = N / 2;
  const uint32_t cp = (uint32_t)cp_len((int)N, 6);
  const uint32_t pos = 14 * N - cp;   // first sample of symbol 13 (its CP): the subframe has 15 N samples
  float2* dst = iq + x.iq_off;
  if (blockIdx.y) {   // symbols 0..12: zeros, one share of the pos samples per workgroup
    const uint32_t per = (pos + SRS_ZERO_PARTS - 1) / SRS_ZERO_PARTS;
    const uint32_t a = (blockIdx.y - 1) * per, b = min(pos, a + per);
    for (uint32_t i = a + t; i < b; i += SRS_THREADS) dst[i] = make_float2(0.0f, 0.0f);
    return;
  }
  // r(k') = exp(j alpha k') rbar_{u,v}(k'), alpha = 2 pi n_cs / 8 (5.5.3.1), zeros up to N / 2; phases in units of pi
  for (uint32_t n = t; n < H; n += SRS_THREADS) {
    float2 z = make_float2(0.0f, 0.0f);
    if (n < x.M_sc) {
      const float cs = (float)((x.n_cs * n) % 8u) * 0.25f;
      const float ph = base_seq_phase(x.nzc, x.q, x.M_sc, n, [cs] { return cs; });
      float sv, cv;
      sincospif(ph, &sv, &cv);
      z = make_float2(cv, sv);
    }
    buf[n] = z;
  }
  __syncthreads();
  // H = 64, 128, 256, 512, 768, 1024 = [3 .] 4^a [. 2]
  uint32_t NS = 1, rem = H;
  if (rem % 3u == 0) {
    pass<3>(buf, H, NS, t);
    NS *= 3;
    rem /= 3;
  }
  while (rem % 4u == 0) {
    pass<4>(buf, H, NS, t);
    NS *= 4;
    rem /= 4;
  }
  if (rem == 2) pass<2>(buf, H, NS, t);
  // the N + CP samples of the symbol: sample n reads the periodic sum at n mod N / 2
  const int twoN = 2 * (int)N, K2 = 2 * x.K + 1;
  const float gN = rsqrtf((float)N) * x.scale * (scale ? scale[blockIdx.x] : 1.0f), rN = 1.0f / (float)N;
  const float f = x.cfo + (cfo ? cfo[blockIdx.x] : 0.0f);
  for (uint32_t i = t; i < N + cp; i += SRS_THREADS) {
    const int n = (int)i - (int)cp;
    const uint32_t nm = (uint32_t)(n + (int)N) % H;
    dst[pos + i] = sc_shift_out(buf[nm], K2, n, twoN, f, pos + i, rN, gN);
  }
}

void launch_srs(const MiSrsTx* txs, uint32_t n_tx, bool last_symbol_only, const float* cfo, const float* scale,
                float2* iq, hipStream_t st) {
  if (!n_tx) return;
  hipLaunchKernelGGL(srs_kernel, dim3(n_tx, last_symbol_only ? 1 : 1 + SRS_ZERO_PARTS), dim3(SRS_THREADS), 0, st, txs,
                     cfo, scale, iq);
}

}  // namespace mi
