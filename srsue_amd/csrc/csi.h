// csi.h -- CSI feedback (CQI / PMI / RI) over a batch's channel estimates: host side of csi.hip.
#pragma once
#include <vector>

#include "csi_body.h"
#include "engine.h"
#include "kernels.h"

namespace mi {

// one workgroup per descriptor; records indexed by batch entry (n_sf of them); noise: per-entry values or nullptr =
// the chest metrics; compact: the estimates are the 4 pilot rows per port
void launch_csi(const float2* ce, const float* metrics, const float* noise, const MiCsiSf* sfs, uint32_t n_phys,
                mi_dl_csi_result_t* out, bool compact, const RxPlanes& rx, uint32_t n_sf, hipStream_t st);

struct CsiEngine {
  std::vector<MiCsiSf> sfs;          // the physical subframes of the plan it was built from
  std::vector<uint64_t> ce_off;      // per entry, to recognise a re-planned batch
  size_t ce_elems = 0;
  DevBuf d_sfs, d_out, d_noise;
  int build(const Plan& P);          // host only
  int upload();                      // blocking
  bool matches(const Plan& P) const;
};

}  // namespace mi
