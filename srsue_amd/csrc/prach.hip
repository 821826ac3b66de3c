// prach.hip -- PRACH preambles of formats 0-3 on gfx950 (36.211 5.7.2, 5.7.3; N_ZC = 839, FDD).
//
//   prach_root_kernel  one workgroup row per distinct root u of the plan: x_u(n) = exp(-j pi u n (n + 1) / 839) and
//                      the 839 twiddles in LDS, X_u(k) = (1 / sqrt(839)) sum_n x_u(n) exp(-j 2 pi n k / 839) by the
//                      direct sum, 4 lanes per k (every fourth term each, added by two shuffles), the twiddle index
//                      n k mod 839 advanced in integers.  |X_u(k)| = 1.
//   prach_gen_kernel   the N_ifft = 1536 L point inverse transform in polyphase form: output sample t = L m + r is
//                      (1 / sqrt(N_ifft)) IDFT_1536 over m of Z_r, with Z_r[(first_bin + k) mod 1536] =
//                      X_u(k) exp(j 2 pi C_v k / 839) exp(j 2 pi ((first_bin + k) r mod N_ifft) / N_ifft) and zeros
//                      elsewhere (839 < 1536: no two bins meet).  A workgroup owns rpw = 1, 2 or 4 adjacent residues
//                      of one transmission: each is one 1536 = 3 . 8 . 8 . 8 point Stockham transform in LDS (12 KiB
//                      per buffer, twiddles from a 1536-entry table), and the results of all rpw stay in LDS until the
//                      output stage, so that rpw adjacent lanes write 8 rpw contiguous bytes.  The output stage
//                      writes the CP (the last N_cp samples), the sequence once (formats 0 / 1) or twice (2 / 3), and
//                      applies the frequency shift and the scale.
// Every phase is reduced in integers before it meets sincospif; the frequency shift cfo i / N_ul is reduced in
// double precision (i reaches 70,175).
#include <hip/hip_runtime.h>

#include "prach.h"
#include "ul_seq_dev.h"

namespace mi {
namespace {

constexpr uint32_t NZC = PRACH_NZC, NF = PRACH_NFFT, T = PRACH_THREADS;
constexpr uint32_t RSTRIDE = NF + 8;     // result rows 16 banks apart: the rpw rows of one output run do not collide
constexpr uint32_t ROOT_PARTS = 4;       // lanes that share one bin of the root's DFT
constexpr uint32_t ROOT_K = T / ROOT_PARTS;                    // 64 bins per workgroup
constexpr uint32_t ROOT_SPLIT = (NZC + ROOT_K - 1) / ROOT_K;   // 14 workgroups per root

// exp(j 2 pi num / den), 0 <= num < den < 2^24
__device__ __forceinline__ float2 unit(uint32_t num, uint32_t den) {
  float s, c;
  sincospif(2.0f * (float)num / (float)den, &s, &c);
  return make_float2(c, s);
}

// unnormalised inverse DFT of 8 points in registers (exp(+j ...)), on the shared 4-point one and beside the 3-point one
using mi::idft;
__device__ __forceinline__ void idft(float2 (&v)[8]) {
  idft4(v[0], v[2], v[4], v[6]);   // E(k) in v[0], v[2], v[4], v[6]
  idft4(v[1], v[3], v[5], v[7]);   // O(k) in v[1], v[3], v[5], v[7]
  const float r = 0.70710678118654752f;
  const float2 o0 = v[1], o1 = make_float2(r * (v[3].x - v[3].y), r * (v[3].x + v[3].y)), o2 = mulj(v[5]),
               o3 = make_float2(-r * (v[7].x + v[7].y), r * (v[7].x - v[7].y));
  const float2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
  v[0] = cadd(e0, o0);
  v[1] = cadd(e1, o1);
  v[2] = cadd(e2, o2);
  v[3] = cadd(e3, o3);
  v[4] = csub(e0, o0);
  v[5] = csub(e1, o1);
  v[6] = csub(e2, o2);
  v[7] = csub(e3, o3);
}

// one Stockham pass of radix R after NS = the product of the earlier radices: butterfly j reads in[j + r NF / R]
// (contiguous over lanes), twiddles by W^(r (j mod NS) NF / (NS R)) < NF, and writes out[(j / NS) NS R + j mod NS + r NS]
template <uint32_t R, uint32_t NS>
__device__ __forceinline__ void pass(const float2* __restrict__ in, float2* __restrict__ out,
                                     const float2* __restrict__ tw, uint32_t t) {
  constexpr uint32_t NB = NF / R;
  for (uint32_t j = t; j < NB; j += T) {
    float2 v[R];
#pragma unroll
    for (uint32_t r = 0; r < R; r++) v[r] = in[j + r * NB];
    const uint32_t k = j % NS;
    if (NS > 1) {
      const uint32_t step = k * (NF / (NS * R));
#pragma unroll
      for (uint32_t r = 1; r < R; r++) v[r] = cmul(v[r], tw[r * step]);
    }
    idft(v);
    const uint32_t j0 = (j / NS) * (NS * R) + k;
#pragma unroll
    for (uint32_t r = 0; r < R; r++) out[j0 + r * NS] = v[r];
  }
}

}  // namespace

__global__ __launch_bounds__(PRACH_THREADS) void prach_root_kernel(const uint32_t* __restrict__ roots,
                                                                   float2* __restrict__ X) {
  __shared__ float2 xu[NZC], tw[NZC];
  const uint32_t u = roots[blockIdx.x], t = threadIdx.x;
  for (uint32_t n = t; n < NZC; n += T) {
    // u n (n + 1) < 838 . 838 . 839 < 2^30, reduced mod 2 . 839 (the phase is in units of pi / 839)
    const uint32_t a = (u * n * (n + 1)) % (2 * NZC);
    float s, c;
    sincospif(-(float)a / (float)NZC, &s, &c);
    xu[n] = make_float2(c, s);
    sincospif(-2.0f * (float)n / (float)NZC, &s, &c);
    tw[n] = make_float2(c, s);
  }
  __syncthreads();
  // 4 adjacent lanes share bin k: lane `part` adds the terms n = part, part + 4, ..., its index n k mod 839 advancing
  // by 4 k mod 839; lanes past the last bin repeat it and store nothing (every lane takes part in the shuffles)
  const uint32_t part = t % ROOT_PARTS, kq = blockIdx.y * ROOT_K + t / ROOT_PARTS;
  const uint32_t k = kq < NZC ? kq : NZC - 1, step = (ROOT_PARTS * k) % NZC;
  float2 acc = make_float2(0.0f, 0.0f);
  uint32_t idx = (part * k) % NZC;
  for (uint32_t n = part; n < NZC; n += ROOT_PARTS) {
    const float2 p = cmul(xu[n], tw[idx]);
    acc.x += p.x;
    acc.y += p.y;
    idx += step;
    idx = idx >= NZC ? idx - NZC : idx;
  }
  acc.x += __shfl_xor(acc.x, 1);
  acc.y += __shfl_xor(acc.y, 1);
  acc.x += __shfl_xor(acc.x, 2);
  acc.y += __shfl_xor(acc.y, 2);
  const float g = rsqrtf((float)NZC);
  if (part == 0 && kq < NZC) X[(size_t)blockIdx.x * NZC + kq] = make_float2(acc.x * g, acc.y * g);
}

// dynamic LDS: tw[NF], B[NF], R[rpw][RSTRIDE] (float2)
__global__ __launch_bounds__(PRACH_THREADS) void prach_gen_kernel(const MiPrachTx* __restrict__ txs,
                                                                  const MiPrachItem* __restrict__ items,
                                                                  const float2* __restrict__ X,
                                                                  const float* __restrict__ cfo,
                                                                  const float* __restrict__ scale,
                                                                  float2* __restrict__ iq) {
  extern __shared__ float2 prach_lds[];
  float2* tw = prach_lds;
  float2* B = tw + NF;
  float2* R = B + NF;
  const MiPrachItem it = items[blockIdx.x];
  const MiPrachTx x = txs[it.tx];
  const uint32_t t = threadIdx.x, rpw = it.rpw;
  for (uint32_t j = t; j < NF; j += T) tw[j] = unit(j, NF);
  const float2* Xu = X + (size_t)x.root_slot * NZC;
  const uint32_t fb = x.first_bin % NF;
  for (uint32_t q = 0; q < rpw; q++) {
    const uint32_t r = it.r0 + q;
    float2* Rq = R + q * RSTRIDE;
    // Z_r in natural order: entry p holds bin first_bin + k with k = (p - first_bin) mod 1536, zero for k >= 839
    for (uint32_t p = t; p < NF; p += T) {
      const uint32_t k = (p + NF - fb) % NF;
      float2 z = make_float2(0.0f, 0.0f);
      if (k < NZC) {
        uint32_t b = x.first_bin + k;
        b = b >= x.N_ifft ? b - x.N_ifft : b;
        z = cmul(cmul(Xu[k], unit((x.C_v * k) % NZC, NZC)), unit((b * r) % x.N_ifft, x.N_ifft));
      }
      Rq[p] = z;
    }
    __syncthreads();   // also orders the twiddle table before its first use
    pass<3, 1>(Rq, B, tw, t);
    __syncthreads();
    pass<8, 3>(B, Rq, tw, t);
    __syncthreads();
    pass<8, 24>(Rq, B, tw, t);
    __syncthreads();
    pass<8, 192>(B, Rq, tw, t);
  }
  __syncthreads();
  // output: rpw adjacent lanes hold the rpw adjacent samples L m + r0 .. of one m
  const float g = rsqrtf((float)x.N_ifft) * (scale ? scale[it.tx] : 1.0f);
  const float f = cfo ? cfo[it.tx] : 0.0f;
  const double fs = (double)f / (double)x.N_ul;
  float2* dst = iq + x.iq_off;
  const uint32_t lg = rpw == 4 ? 2 : rpw == 2 ? 1 : 0, cp0 = x.N_ifft - x.N_cp;
  for (uint32_t e = t; e < NF * rpw; e += T) {
    const uint32_t m = e >> lg, q = e & (rpw - 1), ts = x.L * m + it.r0 + q;
    const float2 s = R[q * RSTRIDE + m];
    const float2 v = make_float2(s.x * g, s.y * g);
    // the copies of sequence sample ts: in the CP (if it is one of the last N_cp), and in each repetition
    uint32_t pos[3], n = 0;
    if (ts >= cp0) pos[n++] = ts - cp0;
    pos[n++] = x.N_cp + ts;
    if (x.reps == 2) pos[n++] = x.N_cp + x.N_ifft + ts;
    for (uint32_t c = 0; c < n; c++) {
      float2 y = v;
      if (f != 0.0f) {   // exp(j 2 pi cfo i / N_ul), i counted from the first CP sample
        double ph = fs * (double)pos[c];
        ph -= floor(ph);
        float sv, cv;
        sincospif(2.0f * (float)ph, &sv, &cv);
        y = cmul(v, make_float2(cv, sv));
      }
      dst[pos[c]] = y;
    }
  }
}

uint32_t prach_gen_lds_bytes(uint32_t rpw) { return (2 * NF + rpw * RSTRIDE) * (uint32_t)sizeof(float2); }

void launch_prach(const uint32_t* roots, uint32_t n_roots, float2* X, const MiPrachTx* txs, const MiPrachItem* items,
                  uint32_t n_items, uint32_t max_rpw, const float* cfo, const float* scale, float2* iq, hipStream_t st) {
  if (!n_items || !n_roots) return;
  static bool attr = false;   // idempotent; the attribute is per function
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&prach_gen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)prach_gen_lds_bytes(PRACH_RPW_MAX));
    attr = true;
  }
  hipLaunchKernelGGL(prach_root_kernel, dim3(n_roots, ROOT_SPLIT), dim3(PRACH_THREADS), 0, st, roots, X);
  hipLaunchKernelGGL(prach_gen_kernel, dim3(n_items), dim3(PRACH_THREADS), prach_gen_lds_bytes(max_rpw), st, txs, items,
                     X, cfo, scale, iq);
}

}  // namespace mi
