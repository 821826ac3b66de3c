// srs_batch.cpp -- C ABI of the batched SRS transmitter (include/mi_ul.h): plan once, upload the table, enqueue
// srs_kernel per run.
#include "srs_engine.h"

struct mi_srs_batch {
  mi::SrsEngine eng;
};

extern "C" {

mi_srs_batch_t* mi_srs_batch_create(const mi_srs_cfg_t* cfgs, uint32_t n, uint32_t flags) {
  if (!cfgs || !n) { mi::set_error("empty SRS batch"); return nullptr; }
  auto* b = new mi_srs_batch();
  b->eng.last_symbol_only = (flags & MI_SRS_FLAG_LAST_SYMBOL_ONLY) != 0;
  // every configuration is checked before anything reaches the device
  if (b->eng.plan.build(cfgs, n) || b->eng.upload(nullptr) ||
      !mi::hip_ok(hipStreamSynchronize(nullptr), "srs upload sync")) {
    delete b;
    return nullptr;
  }
  return b;
}
void mi_srs_batch_destroy(mi_srs_batch_t* b) { delete b; }
size_t mi_srs_batch_iq_offset(const mi_srs_batch_t* b, uint32_t i) {
  return i < b->eng.plan.txs.size() ? b->eng.plan.txs[i].iq_off : 0;
}
size_t mi_srs_batch_iq_samples(const mi_srs_batch_t* b) { return b->eng.plan.iq_samples; }
int mi_srs_batch_run(mi_srs_batch_t* b, const float* d_cfo, const float* d_scale, void* d_iq, void* stream) {
  if (!b || !d_iq) { mi::set_error("null device buffer"); return -1; }
  return b->eng.run(d_cfo, d_scale, d_iq, reinterpret_cast<hipStream_t>(stream));
}
int mi_srs_batch_resource(const mi_srs_batch_t* b, uint32_t i, mi_srs_res_t* r) {
  if (!b || !r || i >= b->eng.plan.res.size()) { mi::set_error("transmission index"); return -1; }
  *r = b->eng.plan.res[i];
  return 0;
}

}  // extern "C"
