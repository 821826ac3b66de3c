// pbch.hip -- PBCH receiver on the GPU (36.211 6.6, 36.212 5.3.1): what srsUE reaches through
// srslte_ue_mib_decode / srslte_pbch_decode (srsUE ue/src/phy/phch_recv.cc:246-253), batched over
// the grid and channel estimates a batch's front end left in HBM.  The arithmetic is the PDCCH path's
// (ctrl_dev.h; contract oracle/o_ctrl.c): decisions are bit-identical on identical soft bits.
//
// MI355X layout:
//   * pbch_llr_kernel: one workgroup per PBCH frame (a subframe 0).  Threads 0..239 equalise one RE each
//     under the 1-port hypothesis, the next 120 one SFBC RE pair each under the 2-port hypothesis; both
//     write their QPSK soft bits, NOT descrambled (the 40 ms phase is unknown), to llr[frame][hyp][480];
//   * pbch_decode_kernel: one wavefront per (candidate, ports, frames combined, phase) job.  Lanes own coded
//     bits for the rate de-matching: a bit's 16 repetitions in the 1920-bit TTI are read straight from the
//     frames that are present, descrambled with the phase's Gold bits and summed in increasing k (an absent
//     quarter adds nothing, as its zeros would); then the 64 lanes are the 64 trellis states of the
//     tail-biting Viterbi and lane 0 traces back and checks the CRC16 against the hypothesis's mask.
//     A job is ~5 KB of reads and 120 trellis steps: the launch is sized by the job count, thousands of
//     candidates x up to 20 jobs per launch, not by the speed of one job.
#include "ctrl_dev.h"
#include "kernels.h"
#include "pbch.h"

namespace mi {

constexpr int PBCH_LLR_T = 256;

__global__ __launch_bounds__(PBCH_LLR_T) void pbch_llr_kernel(const float2* __restrict__ grid,
                                                             const float2* __restrict__ ce,
                                                             const MiPbchFrame* __restrict__ frames,
                                                             const uint32_t* __restrict__ cdata, float* __restrict__ llr,
                                                             float noise) {
  const MiPbchFrame d = frames[blockIdx.x];
  const float2* g = grid + d.grid_off;
  const float2* c0 = ce + d.ce_off;
  const float2* c1 = c0 + d.plane;
  const uint32_t* re = cdata + d.re_off;
  float* o = llr + (size_t)blockIdx.x * 2 * PBCH_BITS;
  for (uint32_t i = threadIdx.x; i < PBCH_RE + PBCH_RE / 2; i += PBCH_LLR_T) {
    if (i < PBCH_RE) {
      float2 x;
      float l[2];
      eq_tm1(g[re[i]], c0[re[i]], noise, x);
      qpsk_llr(x, l);
      reinterpret_cast<float2*>(o)[i] = make_float2(l[0], l[1]);   // 8 B per lane, consecutive
    } else {
      const uint32_t j = 2 * (i - PBCH_RE);
      float4* o2 = reinterpret_cast<float4*>(o + PBCH_BITS + 2 * j);   // 16 B per lane, consecutive, aligned
      if (d.ports == 2) {
        const uint32_t ra = re[j], rb = re[j + 1];
        float2 x0, x1;
        float l0[2], l1[2];
        eq_tm2(g[ra], g[rb], c0[ra], c0[rb], c1[ra], c1[rb], x0, x1);
        qpsk_llr(x0, l0);
        qpsk_llr(x1, l1);
        *o2 = make_float4(l0[0], l0[1], l1[0], l1[1]);
      } else {   // no second port estimated: the hypothesis has no jobs, its row stays defined
        *o2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
  }
}

__global__ __launch_bounds__(64) void pbch_decode_kernel(const float* __restrict__ llr, const MiPbchJob* __restrict__ jobs,
                                                        const uint32_t* __restrict__ cdata, uint32_t rank_off,
                                                        MiPbchRes* __restrict__ res) {
  __shared__ float d[3 * PBCH_D];
  __shared__ uint64_t surv[3 * PBCH_D];
  __shared__ uint8_t c[PBCH_D];
  const MiPbchJob* jp = jobs + blockIdx.x;
  const uint32_t t = threadIdx.x, f = jp->f, ph0 = jp->phase0;
  const uint32_t* scr = cdata + jp->scr_off;
  const uint32_t* rank = cdata + rank_off;
  // rate de-matching (36.212 5.1.4.2, D = 40): coded bit p receives e_k for k = rank(p) + 120 m, m = 0..15,
  // summed in increasing k; e_k of quarter k / 480 comes from the frame at that phase, if the job has it
  for (uint32_t p = t; p < 3 * PBCH_D; p += 64) {
    float s = 0.0f;
    for (uint32_t k = rank[p]; k < PBCH_E; k += 3 * PBCH_D) {
      const uint32_t q = k / PBCH_BITS;
      if (q < ph0 || q >= ph0 + f) continue;
      const float v = llr[jp->llr_off[q - ph0] + (k - q * PBCH_BITS)];
      s = s + (((scr[k >> 5] >> (k & 31u)) & 1u) ? -v : v);
    }
    d[p] = s;
  }
  __syncthreads();
  const uint32_t x = viterbi_tb_crc16(d, PBCH_D, PBCH_A, surv, c);
  if (t == 0) {
    MiPbchRes r;
    r.found = x == jp->mask;
    r.bits = 0;
    for (uint32_t i = 0; i < PBCH_A; i++) r.bits |= (uint32_t)c[i] << (PBCH_A - 1 - i);
    res[blockIdx.x] = r;
  }
}

void launch_pbch_llr(const float2* grid, const float2* ce, const MiPbchFrame* frames, const uint32_t* cdata, float* llr,
                     uint32_t n_frames, float noise, hipStream_t st) {
  if (!n_frames) return;
  hipLaunchKernelGGL(pbch_llr_kernel, dim3(n_frames), dim3(PBCH_LLR_T), 0, st, grid, ce, frames, cdata, llr, noise);
}
void launch_pbch_decode(const float* llr, const MiPbchJob* jobs, const uint32_t* cdata, uint32_t rank_off,
                        MiPbchRes* res, uint32_t n_jobs, hipStream_t st) {
  if (!n_jobs) return;
  hipLaunchKernelGGL(pbch_decode_kernel, dim3(n_jobs), dim3(64), 0, st, llr, jobs, cdata, rank_off, res);
}

}  // namespace mi
