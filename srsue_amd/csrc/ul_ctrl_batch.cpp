// ul_ctrl_batch.cpp -- C ABI of the batched PUCCH, PRACH and SRS transmitters (include/mi_ul.h): plan once, upload
// the tables, enqueue the channel's kernels per run (pucch_kernel with the caller's UCI words; prach_root_kernel +
// prach_gen_kernel; srs_kernel).
#include "prach_engine.h"
#include "pucch_engine.h"
#include "srs_engine.h"
#include "tx_batch.h"

struct mi_pucch_batch { mi::PucchEngine eng; };
struct mi_prach_batch { mi::PrachEngine eng; };
struct mi_srs_batch { mi::SrsEngine eng; };

extern "C" {

mi_pucch_batch_t* mi_pucch_batch_create(const mi_pucch_cfg_t* cfgs, uint32_t n, uint32_t /*flags*/) {
  return mi::tx_batch_create<mi_pucch_batch>(cfgs, n, "empty PUCCH batch", "pucch upload sync",
                                             [](mi_pucch_batch&) {});
}
void mi_pucch_batch_destroy(mi_pucch_batch_t* b) { delete b; }
size_t mi_pucch_batch_iq_offset(const mi_pucch_batch_t* b, uint32_t i) { return mi::tx_batch_iq_offset(b, i); }
size_t mi_pucch_batch_iq_samples(const mi_pucch_batch_t* b) { return b->eng.plan.iq_samples; }
int mi_pucch_batch_run(mi_pucch_batch_t* b, const uint32_t* d_uci, void* d_iq, void* stream) {
  if (!b || !d_uci || !d_iq) { mi::set_error("null device buffer"); return -1; }
  return b->eng.run(d_uci, d_iq, reinterpret_cast<hipStream_t>(stream));
}
int mi_pucch_batch_resource(const mi_pucch_batch_t* b, uint32_t i, mi_pucch_res_t* r) {
  return mi::tx_batch_resource(b, i, r);
}

mi_prach_batch_t* mi_prach_batch_create(const mi_prach_cfg_t* cfgs, uint32_t n, uint32_t flags) {
  return mi::tx_batch_create<mi_prach_batch>(cfgs, n, "empty PRACH batch", "prach upload sync",
                                             [flags](mi_prach_batch& b) {
                                               if (flags & MI_PRACH_FLAG_SINGLE_RESIDUE) b.eng.plan.rpw_cap = 1;
                                             });
}
void mi_prach_batch_destroy(mi_prach_batch_t* b) { delete b; }
size_t mi_prach_batch_iq_offset(const mi_prach_batch_t* b, uint32_t i) { return mi::tx_batch_iq_offset(b, i); }
size_t mi_prach_batch_iq_samples(const mi_prach_batch_t* b) { return b->eng.plan.iq_samples; }
int mi_prach_batch_run(mi_prach_batch_t* b, const float* d_cfo, const float* d_scale, void* d_iq, void* stream) {
  if (!b || !d_iq) { mi::set_error("null device buffer"); return -1; }
  return b->eng.run(d_cfo, d_scale, d_iq, reinterpret_cast<hipStream_t>(stream));
}
int mi_prach_batch_resource(const mi_prach_batch_t* b, uint32_t i, mi_prach_res_t* r) {
  return mi::tx_batch_resource(b, i, r);
}

mi_srs_batch_t* mi_srs_batch_create(const mi_srs_cfg_t* cfgs, uint32_t n, uint32_t flags) {
  return mi::tx_batch_create<mi_srs_batch>(cfgs, n, "empty SRS batch", "srs upload sync", [flags](mi_srs_batch& b) {
    b.eng.last_symbol_only = (flags & MI_SRS_FLAG_LAST_SYMBOL_ONLY) != 0;
  });
}
void mi_srs_batch_destroy(mi_srs_batch_t* b) { delete b; }
size_t mi_srs_batch_iq_offset(const mi_srs_batch_t* b, uint32_t i) { return mi::tx_batch_iq_offset(b, i); }
size_t mi_srs_batch_iq_samples(const mi_srs_batch_t* b) { return b->eng.plan.iq_samples; }
int mi_srs_batch_run(mi_srs_batch_t* b, const float* d_cfo, const float* d_scale, void* d_iq, void* stream) {
  if (!b || !d_iq) { mi::set_error("null device buffer"); return -1; }
  return b->eng.run(d_cfo, d_scale, d_iq, reinterpret_cast<hipStream_t>(stream));
}
int mi_srs_batch_resource(const mi_srs_batch_t* b, uint32_t i, mi_srs_res_t* r) {
  return mi::tx_batch_resource(b, i, r);
}

}  // extern "C"
