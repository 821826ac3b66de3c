// ue_prach.cpp -- the PRACH calls of srsUE's prach.cc (init_cell: init + 64 x gen; is_ready_to_send: send_tti;
// send: CFO shift + scale) under the library's own names and in srsLTE's argument order (include/srslte/srslte.h),
// backed by the GPU generator of prach.hip.
//
// Per srslte_prach_t instance: one HIP stream, the cell's 64 preambles planned and generated in one launch by the
// first mi_prach_gen of a frequency offset and kept on the device (each gen is then one copy), and a
// one-transmission plan for mi_prach_gen_cfo, which generates the preamble with the frequency shift and the scale
// applied in the output stage.
#include <string.h>

#include "../../include/srslte/srslte.h"
#include "prach_engine.h"
#include "../../include/mi_ul.h"

struct mi_prach_ctx {
  hipStream_t st = nullptr;
  mi::PrachEngine cell, one;
  mi::DevBuf d_cell_iq, d_one_iq, d_par;
  float* h_par = nullptr;    // page-locked {cfo, scale} of gen_cfo
  cf_t* h_iq = nullptr;      // page-locked staging of one preamble (srsUE's buffers are pageable)
  mi_prach_cfg_t cfg{};      // the cell: nof_prb, config_idx (16 format), root, zero_corr_zone, high_speed
  size_t len = 0;            // N_cp + N_seq
  int cell_fo = -1;          // frequency offset of the preambles held in d_cell_iq
  ~mi_prach_ctx() {
    if (st) (void)hipStreamSynchronize(st);
    if (h_par) (void)hipHostFree(h_par);
    if (h_iq) (void)hipHostFree(h_iq);
    if (st) (void)hipStreamDestroy(st);
  }
  // one preamble from device memory to the caller's buffer
  int fetch(const void* d_src, cf_t* signal) {
    if (!mi::hip_ok(hipMemcpyAsync(h_iq, d_src, len * 8, hipMemcpyDeviceToHost, st), "D2H preamble") ||
        !mi::hip_ok(hipStreamSynchronize(st), "prach sync"))
      return SRSLTE_ERROR;
    memcpy(signal, h_iq, len * 8);
    return SRSLTE_SUCCESS;
  }
};

extern "C" {

int mi_prach_init(srslte_prach_t* p, uint32_t N_ifft_ul, uint32_t preamble_format, uint32_t root_seq_index,
                  bool high_speed_flag, uint32_t zero_corr_zone_config) {
  if (!p) return SRSLTE_ERROR_INVALID_INPUTS;
  p->impl = nullptr;
  uint32_t nof_prb = 0;
  for (uint32_t b = 6; b <= 100; b++)
    if (mi::std_nof_prb(b) && (uint32_t)mi::symbol_sz(b) == N_ifft_ul) nof_prb = b;
  if (!nof_prb) { mi::set_error("PRACH: N_ifft_ul must be the symbol size of 6, 15, 25, 50, 75 or 100 PRB"); return SRSLTE_ERROR; }
  if (preamble_format > 3) { mi::set_error("PRACH: preamble formats 0-3 only (FDD)"); return SRSLTE_ERROR; }
  // the whole configuration is checked on the host (preamble 0, offset 0) before anything touches the device
  mi_prach_cfg_t c{};
  c.nof_prb = nof_prb;
  c.config_idx = 16 * preamble_format;   // row 0 of the format: only the format enters the waveform
  c.root_seq_idx = root_seq_index;
  c.zero_corr_zone = zero_corr_zone_config;
  c.high_speed = high_speed_flag ? 1 : 0;
  mi_prach_res_t r;
  if (mi_prach_resource(&c, &r)) return SRSLTE_ERROR;
  auto* x = new mi_prach_ctx();
  x->cfg = c;
  x->len = (size_t)r.N_cp + r.N_seq;
  if (!mi::hip_ok(hipStreamCreateWithFlags(&x->st, hipStreamNonBlocking), "stream") || !x->d_par.ensure(2 * sizeof(float)) ||
      !x->d_one_iq.ensure(x->len * 8) ||
      !mi::hip_ok(hipHostMalloc(reinterpret_cast<void**>(&x->h_par), 2 * sizeof(float), hipHostMallocDefault), "pinned") ||
      !mi::hip_ok(hipHostMalloc(reinterpret_cast<void**>(&x->h_iq), x->len * 8, hipHostMallocDefault), "pinned")) {
    delete x;
    return SRSLTE_ERROR;
  }
  p->N_seq = r.N_seq;
  p->N_cp = r.N_cp;
  p->impl = x;
  return SRSLTE_SUCCESS;
}

int mi_prach_free(srslte_prach_t* p) {
  if (!p || !p->impl) return SRSLTE_SUCCESS;
  delete static_cast<mi_prach_ctx*>(p->impl);
  p->impl = nullptr;
  return SRSLTE_SUCCESS;
}

uint32_t mi_prach_get_preamble_format(uint32_t config_idx) {
  const int f = mi_prach_format(config_idx);
  return f < 0 ? 0xFFFFFFFFu : (uint32_t)f;
}

int mi_prach_gen(srslte_prach_t* p, uint32_t seq_index, uint32_t freq_offset, cf_t* signal) {
  if (!p || !p->impl || !signal) return SRSLTE_ERROR_INVALID_INPUTS;
  mi_prach_ctx* x = static_cast<mi_prach_ctx*>(p->impl);
  if (seq_index > 63) { mi::set_error("PRACH: preamble index must be 0..63"); return SRSLTE_ERROR; }
  if (x->cell_fo != (int)freq_offset) {
    // all 64 preambles of the cell at this offset: one plan, one launch, kept on the device
    mi_prach_cfg_t cfgs[64];
    for (uint32_t i = 0; i < 64; i++) {
      cfgs[i] = x->cfg;
      cfgs[i].freq_offset = freq_offset;
      cfgs[i].preamble_idx = i;
    }
    x->cell_fo = -1;
    if (x->cell.plan.build(cfgs, 64)) return SRSLTE_ERROR;   // rejected on the host: nothing is launched
    if (!x->d_cell_iq.ensure(x->cell.plan.iq_samples * 8) || x->cell.upload(x->st) ||
        x->cell.run(nullptr, nullptr, x->d_cell_iq.p, x->st))
      return SRSLTE_ERROR;
    x->cell_fo = (int)freq_offset;
  }
  return x->fetch(x->d_cell_iq.as<float2>() + x->cell.plan.txs[seq_index].iq_off, signal);
}

int mi_prach_gen_cfo(srslte_prach_t* p, uint32_t seq_index, uint32_t freq_offset, float cfo, float scale, cf_t* signal) {
  if (!p || !p->impl || !signal) return SRSLTE_ERROR_INVALID_INPUTS;
  mi_prach_ctx* x = static_cast<mi_prach_ctx*>(p->impl);
  mi_prach_cfg_t c = x->cfg;
  c.freq_offset = freq_offset;
  c.preamble_idx = seq_index;
  if (x->one.plan.build(&c, 1)) return SRSLTE_ERROR;   // every field checked: nothing is launched on an error
  x->h_par[0] = cfo;     // the previous call's DMA out of h_par ended with its stream sync
  x->h_par[1] = scale;
  float* d_par = x->d_par.as<float>();
  if (!mi::hip_ok(hipMemcpyAsync(d_par, x->h_par, 2 * sizeof(float), hipMemcpyHostToDevice, x->st), "H2D cfo") ||
      x->one.upload(x->st) || x->one.run(d_par, d_par + 1, x->d_one_iq.p, x->st))
    return SRSLTE_ERROR;
  return x->fetch(x->d_one_iq.p, signal);
}

}  // extern "C"
