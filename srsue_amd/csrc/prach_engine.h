// prach_engine.h -- device tables + launch of one PRACH plan (shared by the batched ABI, ul_ctrl_batch.cpp, and the
// per-call mi_prach_gen / mi_prach_gen_cfo, ue_prach.cpp).
#pragma once
#include "engine.h"
#include "prach.h"

namespace mi {
void launch_prach(const uint32_t* roots, uint32_t n_roots, float2* X, const MiPrachTx* txs, const MiPrachItem* items,
                  uint32_t n_items, uint32_t max_rpw, const float* cfo, const float* scale, float2* iq, hipStream_t st);

struct PrachEngine {
  PrachPlan plan;
  DevBuf d_txs, d_items, d_roots, d_X;   // d_X: X_u(k) of every distinct root, rewritten by every run
  uint32_t max_rpw = 1;
  // the plan's tables to the device, on `st`; the host vectors must stay unchanged until the copies have run
  int upload(hipStream_t st) {
    const size_t bt = plan.txs.size() * sizeof(MiPrachTx), bi = plan.items.size() * sizeof(MiPrachItem),
                 br = plan.roots.size() * sizeof(uint32_t);
    if (!bt || !d_txs.ensure(bt) || !d_items.ensure(bi) || !d_roots.ensure(br) ||
        !d_X.ensure(plan.roots.size() * PRACH_NZC * sizeof(float2)))
      return -1;
    max_rpw = 1;
    for (const MiPrachItem& it : plan.items) max_rpw = it.rpw > max_rpw ? it.rpw : max_rpw;
    return hip_ok(hipMemcpyAsync(d_txs.p, plan.txs.data(), bt, hipMemcpyHostToDevice, st), "prach upload") &&
                   hip_ok(hipMemcpyAsync(d_items.p, plan.items.data(), bi, hipMemcpyHostToDevice, st), "prach upload") &&
                   hip_ok(hipMemcpyAsync(d_roots.p, plan.roots.data(), br, hipMemcpyHostToDevice, st), "prach upload")
               ? 0 : -1;
  }
  // d_cfo / d_scale: one device float per transmission, or nullptr (no shift / unit scale)
  int run(const float* d_cfo, const float* d_scale, void* d_iq, hipStream_t st) {
    launch_prach(d_roots.as<uint32_t>(), (uint32_t)plan.roots.size(), d_X.as<float2>(), d_txs.as<MiPrachTx>(),
                 d_items.as<MiPrachItem>(), (uint32_t)plan.items.size(), max_rpw, d_cfo, d_scale,
                 static_cast<float2*>(d_iq), st);
    return hip_ok(hipGetLastError(), "prach launch") ? 0 : -1;
  }
};

}  // namespace mi
