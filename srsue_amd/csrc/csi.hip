// csi.hip -- CSI feedback (CQI / PMI / RI) from the channel estimates the CHEST stage left in HBM (arithmetic and
// conventions: csi_body.h; definitions: include/mi_dl.h).
//
// One 256-thread workgroup per physical subframe (a cw = 1 entry's record is written by its partner's workgroup).
// Wavefront r walks CRS symbol row r (l = 0, 4, 7, 11) of the estimates, its lanes consecutive subcarriers: coalesced
// float2 loads of the 2 antennas x 2 ports, one point per lane and step.  The walk is cut at the subband boundaries
// (uniform multiples of 12 x size subcarriers, so every lane of a wavefront is in the same subband): at each the ten
// accumulators are reduced over the wavefront by shuffles and lane 0 leaves them in LDS.  The rows, then the subbands,
// are added in a fixed order -- no atomics: a run gives the same bits every time -- and the tail derives the 240
// capacity / CQI cells (one per thread) and the decisions, written as one fixed-size record per subframe.
#include "csi.h"
#include "csi_body.h"

namespace mi {

__global__ __launch_bounds__(256) void csi_kernel(const float2* __restrict__ ce, const float* __restrict__ metrics,
                                                 const float* __restrict__ noise_in, const MiCsiSf* __restrict__ sfs,
                                                 mi_dl_csi_result_t* __restrict__ out, uint32_t compact, uint32_t n_rx,
                                                 size_t ce_rx, uint32_t n_sf) {
  __shared__ float part[4][MI_CSI_MAX_SB][CSI_NACC];
  __shared__ float sums[1 + MI_CSI_MAX_SB][CSI_NACC];
  const MiCsiSf d = sfs[blockIdx.x];
  const uint32_t tid = threadIdx.x, row = tid >> 6, lane = tid & 63u;
  const uint32_t mask = csi_valid_mask(d.ports, n_rx);
  float noise;
  if (noise_in) {
    noise = noise_in[d.sf];
  } else {   // metrics [antenna][subframe][5], [3] = noise_estimate
    noise = metrics[(size_t)d.sf * 5 + 3];
    if (n_rx == 2) noise = 0.5f * (noise + metrics[((size_t)n_sf + d.sf) * 5 + 3]);
  }
  noise = fmaxf(noise, 1e-9f);
  const float inv_n = 1.0f / noise;
  // row `row` of [port][14 or 4][W]
  const uint32_t W = d.W, l = compact ? row : (row == 0 ? 0u : row == 1 ? 4u : row == 2 ? 7u : 11u);
  const size_t port = (size_t)(compact ? 4 : NSYMB) * W;
  const float2* c00 = ce + d.ce_off + (size_t)l * W;
  const float2* c01 = c00 + port;
  const float2* c10 = c00 + ce_rx;
  const float2* c11 = c10 + port;
  const bool two_ports = d.ports == 2, two_rx = n_rx == 2;
  const float2 zero = make_float2(0.f, 0.f);
  // chunks: the subbands, or the whole row where the bandwidth has none
  const uint32_t n_chunk = d.n_sb ? d.n_sb : 1u, cw = d.n_sb ? 12u * d.sb_prb : W;
  for (uint32_t c = 0; c < n_chunk; c++) {
    const uint32_t k0 = c * cw, k1 = c + 1 == n_chunk ? W : k0 + cw;
    float acc[CSI_NACC];
#pragma unroll
    for (int i = 0; i < CSI_NACC; i++) acc[i] = 0.f;
    for (uint32_t k = k0 + lane; k < k1; k += 64) {
      const float2 h00 = c00[k];
      const float2 h01 = two_ports ? c01[k] : zero;
      const float2 h10 = two_rx ? c10[k] : zero;
      const float2 h11 = two_ports && two_rx ? c11[k] : zero;
      csi_point(h00, h01, h10, h11, mask, inv_n, acc);
    }
#pragma unroll
    for (int i = 0; i < CSI_NACC; i++) {
      float v = acc[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) part[row][c][i] = v;
    }
  }
  __syncthreads();
  if (tid < n_chunk * CSI_NACC) {
    const uint32_t c = tid / CSI_NACC, i = tid % CSI_NACC;
    sums[1 + c][i] = ((part[0][c][i] + part[1][c][i]) + part[2][c][i]) + part[3][c][i];
  }
  __syncthreads();
  if (tid < CSI_NACC) {
    float w = 0.f;
    for (uint32_t c = 0; c < n_chunk; c++) w += sums[1 + c][tid];
    sums[0][tid] = w;
  }
  __syncthreads();
  mi_dl_csi_result_t* o0 = out + d.sf;
  mi_dl_csi_result_t* o1 = d.dup != 0xFFFFFFFFu ? out + d.dup : nullptr;
  if (tid < CSI_CELLS) {
    csi_cell(tid, sums, d, mask, o0);
    if (o1) csi_cell(tid, sums, d, mask, o1);
  }
  if (tid == 0) {
    csi_decide(sums[0], d, mask, noise, o0);
    if (o1) csi_decide(sums[0], d, mask, noise, o1);
  }
}

void launch_csi(const float2* ce, const float* metrics, const float* noise, const MiCsiSf* sfs, uint32_t n_phys,
                mi_dl_csi_result_t* out, bool compact, const RxPlanes& rx, uint32_t n_sf, hipStream_t st) {
  if (!n_phys) return;
  hipLaunchKernelGGL(csi_kernel, dim3(n_phys), dim3(256), 0, st, ce, metrics, noise, sfs, out, (uint32_t)compact, rx.n,
                     rx.ce, n_sf);
}

}  // namespace mi
