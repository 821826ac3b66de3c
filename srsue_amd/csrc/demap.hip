// demap.hip -- PDSCH RE gather + equalisation + max-log soft demapping + descrambling.
//
// Replaces, inside srslte_pdsch_decode_rnti (/root/reference/ue/src/phy/phch_worker.cc:347-348,
// noise_estimate = 0.01 from :340): srslte_pdsch_get (RE gather), srslte_predecoding_single /
// srslte_predecoding_diversity + layerdemap (TM1 / TM2 SFBC), srslte_demod_soft_demodulate
// (max-log, sigma^2 = 0.5, LLR > 0 => bit 1) and srslte_scrambling_f (c(i) = 1 flips the sign).
//
// One lane per RE (TM1) or per SFBC RE pair (TM2).  The RE list (36.211 6.3.5 mapping order) is
// a per-configuration device table, so grid/ce reads walk consecutive subcarriers and every lane
// writes its Qm LLRs contiguously (float2 stores): the LLR stream leaves fully coalesced.
#include "demap_body.h"
#include "kernels.h"

namespace mi {

// antenna a's grid at g + a g_rx, its estimates at c0 / c1 + a c_rx (the batch's antenna planes)
template <int QM, int NRX>
__device__ __forceinline__ void demap_unit(const MiPdschDesc& pd, uint32_t u, const float2* __restrict__ g,
                                           const float2* __restrict__ c0, const float2* __restrict__ c1,
                                           const uint32_t* __restrict__ re, const uint32_t* __restrict__ scr,
                                           float* __restrict__ e, float noise, size_t g_rx, size_t c_rx) {
  if constexpr (NRX == 1) {   // one antenna: the loads as direct arguments (demap_body.h demap_llr)
    if (pd.tm != 2) {
      const uint32_t r = re[u];
      demap_store<QM>(eq_single(g[r], c0[r], noise), scr, u * QM, e);
    } else {
      const uint32_t ra = re[2 * u], rb = re[2 * u + 1];
      float2 x0, x1;
      eq_sfbc(g[ra], g[rb], c0[ra], c0[rb], c1[ra], c1[rb], &x0, &x1);
      demap_store<QM>(x0, scr, 2 * u * QM, e);
      demap_store<QM>(x1, scr, (2 * u + 1) * QM, e);
    }
  } else if (pd.tm != 2) {
    const uint32_t r = re[u];
    EqIn d;
    d.r0 = g[r];
    d.h00 = c0[r];
    EqAcc<false> acc = eq_terms<false>(d);
#pragma unroll
    for (int a = 1; a < NRX; a++) {
      d.r0 = g[a * g_rx + r];
      d.h00 = c0[a * c_rx + r];
      eq_add<false>(acc, d);
    }
    float2 x;
    eq_finish<false>(acc, noise, &x, nullptr);
    demap_store<QM>(x, scr, u * QM, e);
  } else {
    const uint32_t ra = re[2 * u], rb = re[2 * u + 1];
    EqAcc<true> acc = eq_terms<true>(EqIn{g[ra], g[rb], c0[ra], c0[rb], c1[ra], c1[rb]});
#pragma unroll
    for (int a = 1; a < NRX; a++) {
      const float2 *ga = g + a * g_rx, *p0 = c0 + a * c_rx, *p1 = c1 + a * c_rx;
      eq_add<true>(acc, EqIn{ga[ra], ga[rb], p0[ra], p0[rb], p1[ra], p1[rb]});
    }
    float2 x0, x1;
    eq_finish<true>(acc, noise, &x0, &x1);
    demap_store<QM>(x0, scr, 2 * u * QM, e);
    demap_store<QM>(x1, scr, (2 * u + 1) * QM, e);
  }
}

// NRX receive antennas combined per unit (demap_body.h eq_terms / eq_add / eq_finish); the antenna planes' strides are launch arguments
template <int NRX>
__global__ __launch_bounds__(256) void demap_kernel(const float2* __restrict__ grid, const float2* __restrict__ ce,
                                                   float* __restrict__ e, const MiSfDesc* __restrict__ sfs,
                                                   const MiPdschDesc* __restrict__ pds,
                                                   const MiCellDesc* __restrict__ cells,
                                                   const uint32_t* __restrict__ re_tab,
                                                   const uint32_t* __restrict__ scr_tab, float noise, size_t g_rx,
                                                   size_t c_rx) {
  const MiSfDesc d = sfs[blockIdx.y];
  const MiPdschDesc pd = pds[d.pdsch];
  if (pd.tm > 2) return;   // spatial multiplexing entries: sm_detect_kernel writes their LLRs (sm_detect.hip)
  const uint32_t units = pd.tm == 2 ? pd.nre / 2 : pd.nre;
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const MiCellDesc c = cells[d.cell];
  const float2* g = grid + d.grid_off;
  const float2* c0 = ce + d.ce_off;
  const float2* c1 = c0 + (size_t)NSYMB * c.W;
  const uint32_t* re = re_tab + pd.re_off;
  const uint32_t* scr = scr_tab + pd.scr_off;
  float* out = e + d.e_off;
  switch (pd.Qm) {
    case 2: demap_unit<2, NRX>(pd, u, g, c0, c1, re, scr, out, noise, g_rx, c_rx); break;
    case 4: demap_unit<4, NRX>(pd, u, g, c0, c1, re, scr, out, noise, g_rx, c_rx); break;
    default: demap_unit<6, NRX>(pd, u, g, c0, c1, re, scr, out, noise, g_rx, c_rx); break;
  }
}

void launch_demap(const float2* grid, const float2* ce, float* e, const MiSfDesc* sfs, const MiPdschDesc* pd,
                  const MiCellDesc* cells, const uint32_t* re_tab, const uint32_t* scr, uint32_t n_sf,
                  uint32_t max_units, float noise, const RxPlanes& rx, hipStream_t st) {
  if (!n_sf || !max_units) return;
  dim3 g((max_units + 255) / 256, n_sf);
  if (rx.n == 2)
    hipLaunchKernelGGL(demap_kernel<2>, g, dim3(256), 0, st, grid, ce, e, sfs, pd, cells, re_tab, scr, noise, rx.grid,
                       rx.ce);
  else
    hipLaunchKernelGGL(demap_kernel<1>, g, dim3(256), 0, st, grid, ce, e, sfs, pd, cells, re_tab, scr, noise, rx.grid,
                       rx.ce);
}

}  // namespace mi
