// ul_seq_dev.h -- device code the uplink transmitters share (ul.hip, pucch.hip, srs.hip, prach.hip): the tabulated
// base sequences of 36.211 5.5.1.2, the phase of the base sequence r-bar_{u,v}(n) (5.5.1.1 / 5.5.1.2), complex
// helpers, the register-level inverse 3- and 4-point DFTs and the half-subcarrier rotation of the SC-FDMA output
// (5.6).  Everything is __forceinline__ and takes values, so each kernel compiles as if the code stood in it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {

// 36.211 Tables 5.5.1.2-1 / 5.5.1.2-2: phi(n) of the base sequences r_u(n) = exp(j phi(n) pi / 4) for M_sc = 12
// and 24 (L_prb = 1, 2), sequence-group number u = 0..29.  Transcribed from the specification; the CPU suite
// checks every row's low-PAPR design property (tests/test_oracle_ul.py), the oracle holds its own copy and the GPU
// suite runs every group of both tables against it.
static __constant__ int8_t UL_PHI12[30][12] = {
    {-1,  1,  3, -3,  3,  3,  1,  1,  3,  1, -3,  3},
    { 1,  1,  3,  3,  3, -1,  1, -3, -3,  1, -3,  3},
    { 1,  1, -3, -3, -3, -1, -3, -3,  1, -3,  1, -1},
    {-1,  1,  1,  1,  1, -1, -3, -3,  1, -3,  3, -1},
    {-1,  3,  1, -1,  1, -1, -3, -1,  1, -1,  1,  3},
    { 1, -3,  3, -1, -1,  1,  1, -1, -1,  3, -3,  1},
    {-1,  3, -3, -3, -3,  3,  1, -1,  3,  3, -3,  1},
    {-3, -1, -1, -1,  1, -3,  3, -1,  1, -3,  3,  1},
    { 1, -3,  3,  1, -1, -1, -1,  1,  1,  3, -1,  1},
    { 1, -3, -1,  3,  3, -1, -3,  1,  1,  1,  1,  1},
    {-1,  3, -1,  1,  1, -3, -3, -1, -3, -3,  3, -1},
    { 3,  1, -1, -1,  3,  3, -3,  1,  3,  1,  3,  3},
    { 1, -3,  1,  1, -3,  1,  1,  1, -3, -3, -3,  1},
    { 3,  3, -3,  3, -3,  1,  1,  3, -1, -3,  3,  3},
    {-3,  1, -1, -3, -1,  3,  1,  3,  3,  3, -1,  1},
    { 3, -1,  1, -3, -1, -1,  1,  1,  3,  1, -1, -3},
    { 1,  3,  1, -1,  1,  3,  3,  3, -1, -1,  3, -1},
    {-3,  1,  1,  3, -3,  3, -3, -3,  3,  1,  3, -1},
    {-3,  3,  1,  1, -3,  1, -3, -3, -1, -1,  1, -3},
    {-1,  3,  1,  3,  1, -1, -1,  3, -3, -1, -3, -1},
    {-1, -3,  1,  1,  1,  1,  3,  1, -1,  1, -3, -1},
    {-1,  3, -1,  1, -3, -3, -3, -3, -3,  1, -1, -3},
    { 1,  1, -3, -3, -3, -3, -1,  3, -3,  1, -3,  3},
    { 1,  1, -1, -3, -1, -3,  1, -1,  1,  3, -1,  1},
    { 1,  1,  3,  1,  3,  3, -1,  1, -1, -3, -3,  1},
    { 1, -3,  3,  3,  1,  3,  3,  1, -3, -1, -1,  3},
    { 1,  3, -3, -3,  3, -3,  1, -1, -1,  3, -1, -3},
    {-3, -1, -3, -1, -3,  3,  1, -1,  1,  3, -3, -3},
    {-1,  3, -3,  3, -1,  3,  3, -3,  3,  3, -1, -1},
    { 3, -3, -3, -1, -1, -3, -1,  3, -3,  3,  1, -1}};
static __constant__ int8_t UL_PHI24[30][24] = {
    {-1,  3,  1, -3,  3, -1,  1,  3, -3,  3,  1,  3, -3,  3,  1,  1, -1,  1,  3, -3,  3, -3, -1, -3},
    {-3,  3, -3, -3, -3,  1, -3, -3,  3, -1,  1,  1,  1,  3,  1, -1,  3, -3, -3,  1,  3,  1,  1, -3},
    { 3, -1,  3,  3,  1,  1, -3,  3,  3,  3,  3,  1, -1,  3, -1,  1,  1, -1, -3, -1, -1,  1,  3,  3},
    {-1, -3,  1,  1,  3, -3,  1,  1, -3, -1, -1,  1,  3,  1,  3,  1, -1,  3,  1,  1, -3, -1, -3, -1},
    {-1, -1, -1, -3, -3, -1,  1,  1,  3,  3, -1,  3, -1,  1, -1, -3,  1, -1, -3, -3,  1, -3, -1, -1},
    {-3,  1,  1,  3, -1,  1,  3,  1, -3,  1, -3,  1,  1, -1, -1,  3, -1, -3,  3, -3, -3, -3,  1,  1},
    { 1,  1, -1, -1,  3, -3, -3,  3, -3,  1, -1, -1,  1, -1,  1,  1, -1, -3, -1,  1, -1,  3, -1, -3},
    {-3,  3,  3, -1, -1, -3, -1,  3,  1,  3,  1,  3,  1,  1, -1,  3,  1, -1,  1,  3, -3, -1, -1,  1},
    {-3,  1,  3, -3,  1, -1, -3,  3, -3,  3, -1, -1, -1, -1,  1, -3, -3, -3,  1, -3, -3, -3,  1, -3},
    { 1,  1, -3,  3,  3, -1, -3, -1,  3, -3,  3,  3,  3, -1,  1,  1, -3,  1, -1,  1,  1, -3,  1,  1},
    {-1,  1, -3, -3,  3, -1,  3, -1, -1, -3, -3, -3, -1, -3, -3,  1, -1,  1,  3,  3, -1,  1, -1,  3},
    { 1,  3,  3, -3, -3,  1,  3,  1, -1, -3, -3, -3,  3,  3, -3,  3,  3, -1, -3,  3, -1,  1, -3,  1},
    { 1,  3,  3,  1,  1,  1, -1, -1,  1, -3,  3, -1,  1,  1, -3,  3,  3, -1, -3,  3, -3, -1, -3, -1},
    { 3, -1, -1, -1, -1, -3, -1,  3,  3,  1, -1,  1,  3,  3,  3, -1,  1,  1, -3,  1,  3, -1, -3,  3},
    {-3, -3,  3,  1,  3,  1, -3,  3,  1,  3,  1,  1,  3,  3, -1, -1, -3,  1, -3, -1,  3,  1,  1,  3},
    {-1, -1,  1, -3,  1,  3, -3,  1, -1, -3, -1,  3,  1,  3,  1, -1, -3, -3, -1, -1, -3, -3, -3, -1},
    {-1, -3,  3, -1, -1, -1, -1,  1,  1, -3,  3,  1,  3,  3,  1, -1,  1, -3,  1, -3,  1,  1, -3, -1},
    { 1,  3, -1,  3,  3, -1, -3,  1, -1, -3,  3,  3,  3, -1,  1,  1,  3, -1, -3, -1,  3, -1, -1, -1},
    { 1,  1,  1,  1,  1, -1,  3, -1, -3,  1,  1,  3, -3,  1, -3, -1,  1,  1, -3, -3,  3,  1,  1, -3},
    { 1,  3,  3,  1, -1, -3,  3, -1,  3,  3,  3, -3,  1, -1,  1, -1, -3, -1,  1,  3, -1,  3, -3, -3},
    {-1, -3,  3, -3, -3, -3, -1, -1, -3, -1, -3,  3,  1,  3, -3, -1,  3, -1,  1, -1,  3, -3,  1, -1},
    {-3, -3,  1,  1, -1,  1, -1,  1, -1,  3,  1, -3, -1,  1, -1,  1, -1, -1,  3,  3, -3, -1,  1, -3},
    {-3, -1, -3,  3,  1, -1, -3, -1, -3, -3,  3, -3,  3, -3, -1,  1,  3,  1, -3,  1,  3,  3, -1, -3},
    {-1, -1, -1, -1,  3,  3,  3,  1,  3,  3, -3,  1,  3, -1,  3, -1,  3,  3, -3,  3,  1, -1,  3,  3},
    { 1, -1,  3,  3, -1, -3,  3, -3, -1, -1,  3, -1,  3, -1, -1,  1,  1,  1,  1, -1, -1, -3, -1,  3},
    { 1, -1,  1, -1,  3, -1,  3,  1,  1, -1, -1, -3,  1,  1, -3,  1,  3, -3,  1,  1, -3, -3, -1, -1},
    {-3, -1,  1,  3,  1,  1, -3, -1, -1, -3,  3, -3,  3,  1, -3,  3, -3,  1, -1,  1, -3,  1,  1,  1},
    {-1, -3,  3,  3,  1,  1,  3, -1, -3, -1, -1, -1,  3,  1, -3, -3, -1,  3, -3, -1, -3, -1, -3, -1},
    {-1, -3, -1, -1,  1, -3, -1, -1,  1, -1, -3,  1,  1, -3,  1, -3, -3,  3,  1,  1, -1,  3, -1, -1},
    { 1,  1, -1, -1, -3, -1,  3, -1,  3, -1,  1,  3,  1, -1,  3,  1,  3, -3, -3,  1, -1, -1,  1,  3}};

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 mulj(float2 a) { return make_float2(-a.y, a.x); }   // * j

// phase, in units of pi, of the base sequence r-bar_{u,v}(n) of length M_sc, n < M_sc, plus the caller's cyclic-shift
// phase shift().  nzc != 0: x_q(n mod N_ZC), x_q(m) = exp(-j pi q m (m + 1) / N_ZC), the phase q m (m + 1) mod 2 N_ZC
// reduced in 64-bit integers; nzc == 0: exp(j phi_q(n) pi / 4) of the tabulated group q, M_sc = 12 or 24.  The shift
// is a callable so that it is evaluated inside each branch, where pusch_mod_kernel has its division: hoisted in front
// of the branch, that kernel allocates its registers differently.
template <class Shift>
__device__ __forceinline__ float base_seq_phase(uint32_t nzc, uint32_t q, uint32_t M_sc, uint32_t n, Shift shift) {
  if (nzc) {
    const uint32_t m = n % nzc;
    const uint32_t a = (uint32_t)(((uint64_t)q * m * (m + 1)) % (2ull * nzc));
    return -(float)a / (float)nzc + shift();
  }
  return (float)(M_sc == 12 ? UL_PHI12[q][n] : UL_PHI24[q][n]) * 0.25f + shift();
}

// unnormalised inverse DFTs of 3 and 4 points in registers (exp(+j ...))
__device__ __forceinline__ void idft(float2 (&v)[3]) {
  const float2 t = cadd(v[1], v[2]), d = csub(v[1], v[2]);
  const float2 m = make_float2(v[0].x - 0.5f * t.x, v[0].y - 0.5f * t.y);
  const float h = 0.86602540378443865f;
  const float2 s = make_float2(-h * d.y, h * d.x);
  v[0] = cadd(v[0], t);
  v[1] = cadd(m, s);
  v[2] = csub(m, s);
}
__device__ __forceinline__ void idft4(float2& a0, float2& a1, float2& a2, float2& a3) {
  const float2 s0 = cadd(a0, a2), s1 = csub(a0, a2), s2 = cadd(a1, a3), s3 = mulj(csub(a1, a3));
  a0 = cadd(s0, s2);
  a1 = cadd(s1, s3);
  a2 = csub(s0, s2);
  a3 = csub(s1, s3);
}
__device__ __forceinline__ void idft(float2 (&v)[4]) { idft4(v[0], v[1], v[2], v[3]); }

// sample n (-cp .. N - 1) of an SC-FDMA symbol whose subcarriers start K + 1/2 from the band centre (5.6):
// y exp(j pi (2 K + 1) n / N) g, K2 = 2 K + 1, its argument reduced exactly in integers (|K2 n| < 2^23), times the
// frequency shift srslte_ue_ul_set_cfo asks for (cfo subcarriers over the subframe's sample index idx); rN = 1 / N
__device__ __forceinline__ float2 sc_shift_out(float2 y, int K2, int n, int twoN, float cfo, uint32_t idx, float rN,
                                               float g) {
  int r = (K2 * n) % twoN;
  r = r < 0 ? r + twoN : r;
  float sv, cv;
  sincospif(((float)r + 2.0f * cfo * (float)idx) * rN, &sv, &cv);
  const float2 z = cmul(y, make_float2(cv, sv));
  return make_float2(z.x * g, z.y * g);
}

}  // namespace mi
