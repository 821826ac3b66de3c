// ctrl_dev.h -- device functions shared by the DL control kernels (ctrl.hip) and the PBCH kernels
// (pbch.hip): the equalisers, the QPSK demapper and the tail-biting Viterbi + CRC16 of one wavefront.
// One definition each, so both paths run the same arithmetic (contract: oracle/o_ctrl.c).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctrl_rx_body.h"

namespace mi {

__device__ __forceinline__ void eq_tm1(float2 y, float2 h, float noise, float2& x) {
  const float den = h.x * h.x + h.y * h.y + noise;
  x.x = (y.x * h.x + y.y * h.y) / den;
  x.y = (y.y * h.x - y.x * h.y) / den;
}

// Alamouti / SFBC combining of an RE pair (the PDSCH demapper's arithmetic, demap.hip)
__device__ __forceinline__ void eq_tm2(float2 r0, float2 r1, float2 h00, float2 h01, float2 h10, float2 h11, float2& x0,
                                       float2& x1) {
  float hh = h00.x * h00.x + h00.y * h00.y + h11.x * h11.x + h11.y * h11.y;
  if (hh <= 0.f) hh = 1e-9f;
  const float s = 1.41421356237f / hh;
  x0.x = s * ((h00.x * r0.x + h00.y * r0.y) + (h11.x * r1.x + h11.y * r1.y));
  x0.y = s * ((h00.x * r0.y - h00.y * r0.x) + (h11.y * r1.x - h11.x * r1.y));
  x1.x = s * (-(h10.x * r0.x + h10.y * r0.y) + (h01.x * r1.x + h01.y * r1.y));
  x1.y = s * (-(h10.y * r0.x - h10.x * r0.y) + (h01.x * r1.y - h01.y * r1.x));
}

// the QPSK demapper qpsk_llr: ctrl_rx_body.h (one definition for these kernels and the host emulation)

// generators 133, 171, 165 (octal): bit 6 <-> c_k, bit 0 <-> c_{k-6}
__device__ __forceinline__ int par7(uint32_t x) { return __popc(x) & 1; }

// Tail-biting Viterbi (36.212 5.1.3.1) + CRC16 of one wavefront (workgroup of 64 threads, lane t = trellis
// state t).  d: the 3 D de-matched soft bits d0 | d1 | d2 in LDS, written by this workgroup before the call
// (the caller has synchronised); surv [3 D] and c [D] are LDS scratch.  Three circular copies, the middle one
// kept; largest final metric, lowest state on ties.  On return c holds the D = A + 16 decoded bits (lane 0
// wrote them: only lane 0 may read them without a barrier) and lane 0's return value is the CRC16 (g =
// 0x1021, zero init) of the A payload bits XOR the 16 received CRC bits; other lanes return 0.
__device__ __forceinline__ uint32_t viterbi_tb_crc16(const float* d, uint32_t D, uint32_t A, uint64_t* surv, uint8_t* c) {
  const uint32_t t = threadIdx.x;
  const uint32_t u = t >> 5;
  const uint32_t s0 = (t << 1) & 63u, s1 = s0 | 1u;
  const uint32_t r0 = (u << 6) | s0, r1 = (u << 6) | s1;
  const int o00 = par7(r0 & 0133u), o01 = par7(r0 & 0171u), o02 = par7(r0 & 0165u);
  const int o10 = par7(r1 & 0133u), o11 = par7(r1 & 0171u), o12 = par7(r1 & 0165u);
  float pm = 0.0f;
  for (uint32_t k = 0, kk = 0; k < 3 * D; k++) {
    const float v0 = d[kk], v1 = d[D + kk], v2 = d[2 * D + kk];
    float bm0 = 0.0f, bm1 = 0.0f;
    bm0 = bm0 + (o00 ? v0 : -v0); bm0 = bm0 + (o01 ? v1 : -v1); bm0 = bm0 + (o02 ? v2 : -v2);
    bm1 = bm1 + (o10 ? v0 : -v0); bm1 = bm1 + (o11 ? v1 : -v1); bm1 = bm1 + (o12 ? v2 : -v2);
    const float m0 = __shfl(pm, (int)s0, 64) + bm0;
    const float m1 = __shfl(pm, (int)s1, 64) + bm1;
    const bool pick = m1 > m0;
    pm = pick ? m1 : m0;
    const uint64_t b = __ballot(pick);
    if (t == 0) surv[k] = b;
    if (++kk == D) kk = 0;
  }
  // best final state: largest metric, lowest index on ties
  float bv = pm;
  uint32_t bi = t;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const uint32_t oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  __syncthreads();
  uint32_t x = 0;
  if (t == 0) {
    uint32_t st = bi;
    for (int k = (int)(3 * D) - 1; k >= 0; k--) {
      if ((uint32_t)k >= D && (uint32_t)k < 2 * D) c[k - D] = (uint8_t)(st >> 5);
      st = ((st << 1) & 63u) | (uint32_t)((surv[k] >> st) & 1u);
    }
    uint32_t reg = 0;
    for (uint32_t i = 0; i < A; i++) {
      const uint32_t fb = ((reg >> 15) ^ c[i]) & 1u;
      reg = ((reg << 1) & 0xFFFFu) ^ (fb ? 0x1021u : 0u);
    }
    uint32_t rx = 0;
    for (uint32_t i = 0; i < 16; i++) rx = (rx << 1) | c[A + i];
    x = (reg ^ rx) & 0xFFFFu;
  }
  return x;
}

}  // namespace mi
