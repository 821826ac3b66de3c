// pucch_engine.h -- device tables + launch of one PUCCH plan (shared by the batched ABI, ul_ctrl_batch.cpp, and
// the per-TTI mi_ue_ul_pucch_encode, ue_ul.cpp).
#pragma once
#include "engine.h"
#include "pucch.h"

namespace mi {
void launch_pucch(const MiPucchTx* txs, uint32_t n_tx, const uint32_t* rm, const uint32_t* uci, float2* iq,
                  hipStream_t st);

struct PucchEngine {
  PucchPlan plan;
  DevBuf d_txs, d_rm;
  // the plan's tables to the device, on `st`; the host vectors must stay unchanged until the copy has run
  int upload(hipStream_t st) {
    const size_t b = plan.txs.size() * sizeof(MiPucchTx);
    if (!b || !d_txs.ensure(b) || !d_rm.ensure(sizeof(plan.rm))) return -1;
    return hip_ok(hipMemcpyAsync(d_txs.p, plan.txs.data(), b, hipMemcpyHostToDevice, st), "pucch upload") &&
                   hip_ok(hipMemcpyAsync(d_rm.p, plan.rm, sizeof(plan.rm), hipMemcpyHostToDevice, st), "pucch upload")
               ? 0 : -1;
  }
  int run(const uint32_t* d_uci, void* d_iq, hipStream_t st) {
    launch_pucch(d_txs.as<MiPucchTx>(), (uint32_t)plan.txs.size(), d_rm.as<uint32_t>(), d_uci,
                 static_cast<float2*>(d_iq), st);
    return hip_ok(hipGetLastError(), "pucch launch") ? 0 : -1;
  }
};

}  // namespace mi
