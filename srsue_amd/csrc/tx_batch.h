// tx_batch.h -- what the batched C ABIs of the PUCCH, PRACH and SRS transmitters (include/mi_ul.h, ul_ctrl_batch.cpp)
// have in common: a batch B holds one engine `eng` (pucch_engine.h, prach_engine.h, srs_engine.h), whose plan holds
// txs (each with its iq_off), res and iq_samples.  The run calls differ and stay with each channel.
#pragma once
#include "engine.h"

namespace mi {

// plan once and upload the tables; `setup` applies the create flags to the new batch before it plans
template <class B, class Cfg, class Setup>
B* tx_batch_create(const Cfg* cfgs, uint32_t n, const char* empty_msg, const char* sync_msg, Setup setup) {
  if (!cfgs || !n) { set_error(empty_msg); return nullptr; }
  auto* b = new B();
  setup(*b);
  // every configuration is checked before anything reaches the device
  if (b->eng.plan.build(cfgs, n) || b->eng.upload(nullptr) || !hip_ok(hipStreamSynchronize(nullptr), sync_msg)) {
    delete b;
    return nullptr;
  }
  return b;
}
template <class B>
size_t tx_batch_iq_offset(const B* b, uint32_t i) {
  return i < b->eng.plan.txs.size() ? b->eng.plan.txs[i].iq_off : 0;
}
template <class B, class Res>
int tx_batch_resource(const B* b, uint32_t i, Res* r) {
  if (!b || !r || i >= b->eng.plan.res.size()) { set_error("transmission index"); return -1; }
  *r = b->eng.plan.res[i];
  return 0;
}

}  // namespace mi
