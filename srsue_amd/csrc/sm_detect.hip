// sm_detect.hip -- two-layer spatial multiplexing (TM3 / TM4) detection + max-log soft demapping + descrambling of
// both codewords (arithmetic and conventions: sm_body.h).
//
// One lane per RE of a codeword pair; blockIdx.y = the pair (Plan::sm).  The lane reads its RE of the two antennas'
// grids and the four channel estimates through the RE list (36.211 6.3.5 mapping order, as demap_kernel: consecutive
// lanes walk consecutive subcarriers), detects both layers once, and writes Qm0 LLRs into codeword 0's stream and
// Qm1 into codeword 1's, each contiguous per lane (float2 stores): a streaming pass, 48 B in and 4 (Qm0 + Qm1) B out
// per RE.  Rate de-matching then reads the two streams as those of any two transport blocks.
#include "kernels.h"
#include "sm_body.h"

namespace mi {

__global__ __launch_bounds__(256) void sm_detect_kernel(const float2* __restrict__ grid, const float2* __restrict__ ce,
                                                       float* __restrict__ e, const MiSmDesc* __restrict__ sm,
                                                       const uint32_t* __restrict__ re_tab,
                                                       const uint32_t* __restrict__ scr_tab, float noise, size_t g_rx,
                                                       size_t c_rx) {
  const MiSmDesc d = sm[blockIdx.y];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.nre) return;
  sm_detect_re(d, i, grid + d.goff, ce + d.coff, re_tab, scr_tab, e, noise, g_rx, c_rx);
}

void launch_sm_detect(const float2* grid, const float2* ce, float* e, const MiSmDesc* sm, uint32_t n_pairs,
                      uint32_t max_nre, const uint32_t* re_tab, const uint32_t* scr, float noise, const RxPlanes& rx,
                      hipStream_t st) {
  if (!n_pairs || !max_nre) return;
  hipLaunchKernelGGL(sm_detect_kernel, dim3((max_nre + 255) / 256, n_pairs), dim3(256), 0, st, grid, ce, e, sm, re_tab,
                     scr, noise, rx.grid, rx.ce);
}

}  // namespace mi
