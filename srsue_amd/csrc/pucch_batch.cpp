// pucch_batch.cpp -- C ABI of the batched PUCCH transmitter (include/mi_ul.h): plan once, upload the tables,
// enqueue pucch_kernel per run with the caller's UCI words.
#include "pucch_engine.h"

struct mi_pucch_batch {
  mi::PucchEngine eng;
};

extern "C" {

mi_pucch_batch_t* mi_pucch_batch_create(const mi_pucch_cfg_t* cfgs, uint32_t n, uint32_t /*flags*/) {
  if (!cfgs || !n) { mi::set_error("empty PUCCH batch"); return nullptr; }
  auto* b = new mi_pucch_batch();
  // every configuration is checked before anything reaches the device
  if (b->eng.plan.build(cfgs, n) || b->eng.upload(nullptr) ||
      !mi::hip_ok(hipStreamSynchronize(nullptr), "pucch upload sync")) {
    delete b;
    return nullptr;
  }
  return b;
}
void mi_pucch_batch_destroy(mi_pucch_batch_t* b) { delete b; }
size_t mi_pucch_batch_iq_offset(const mi_pucch_batch_t* b, uint32_t i) {
  return i < b->eng.plan.txs.size() ? b->eng.plan.txs[i].iq_off : 0;
}
size_t mi_pucch_batch_iq_samples(const mi_pucch_batch_t* b) { return b->eng.plan.iq_samples; }
int mi_pucch_batch_run(mi_pucch_batch_t* b, const uint32_t* d_uci, void* d_iq, void* stream) {
  if (!b || !d_uci || !d_iq) { mi::set_error("null device buffer"); return -1; }
  return b->eng.run(d_uci, d_iq, reinterpret_cast<hipStream_t>(stream));
}
int mi_pucch_batch_resource(const mi_pucch_batch_t* b, uint32_t i, mi_pucch_res_t* r) {
  if (!b || !r || i >= b->eng.plan.res.size()) { mi::set_error("transmission index"); return -1; }
  *r = b->eng.plan.res[i];
  return 0;
}

}  // extern "C"
