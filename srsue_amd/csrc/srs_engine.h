// srs_engine.h -- device table + launch of one SRS plan (shared by the batched ABI, ul_ctrl_batch.cpp, and the
// per-TTI mi_ue_ul_srs_encode, ue_ul.cpp).
#pragma once
#include "engine.h"
#include "srs.h"

namespace mi {
void launch_srs(const MiSrsTx* txs, uint32_t n_tx, bool last_symbol_only, const float* cfo, const float* scale,
                float2* iq, hipStream_t st);

struct SrsEngine {
  SrsPlan plan;
  DevBuf d_txs;
  bool last_symbol_only = false;   // MI_SRS_FLAG_LAST_SYMBOL_ONLY
  // the plan's table to the device, on `st`; the host vector must stay unchanged until the copy has run
  int upload(hipStream_t st) {
    const size_t b = plan.txs.size() * sizeof(MiSrsTx);
    if (!b || !d_txs.ensure(b)) return -1;
    return hip_ok(hipMemcpyAsync(d_txs.p, plan.txs.data(), b, hipMemcpyHostToDevice, st), "srs upload") ? 0 : -1;
  }
  // d_cfo / d_scale: one device float per transmission, or nullptr (no shift / unit scale)
  int run(const float* d_cfo, const float* d_scale, void* d_iq, hipStream_t st) {
    launch_srs(d_txs.as<MiSrsTx>(), (uint32_t)plan.txs.size(), last_symbol_only, d_cfo, d_scale,
               static_cast<float2*>(d_iq), st);
    return hip_ok(hipGetLastError(), "srs launch") ? 0 : -1;
  }
};

}  // namespace mi
