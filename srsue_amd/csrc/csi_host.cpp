// csi_host.cpp -- host side of the CSI feedback stage (csi.h) and the mi_dl_csi_* / mi_csi_* C ABI.
#include <string.h>

#include "batch_impl.h"
#include "csi.h"

namespace mi {

int CsiEngine::build(const Plan& P) {
  const size_t n = P.sfs.size();
  sfs.clear();
  ce_off.clear();
  ce_elems = P.ce_elems;
  // the entries that own samples (all but the cw = 1 ones, Plan::phys; empty = every entry), in order
  std::vector<uint8_t> owns(n, P.phys.empty() ? 1 : 0);
  for (uint32_t s : P.phys) owns[s] = 1;
  for (size_t s = 0; s < n; s++) {
    ce_off.push_back(P.sfs[s].ce_off);
    if (!owns[s]) continue;
    const MiCellDesc& c = P.cells[P.sfs[s].cell];
    MiCsiSf d{};
    d.ce_off = P.sfs[s].ce_off;
    d.W = c.W;
    d.ports = c.nof_ports;
    if (c.nof_ports < 1 || c.nof_ports > 2 || !csi_subbands(c.nof_prb, &d.sb_prb, &d.n_sb)) {
      set_error("csi: 1 or 2 CRS ports, 6..110 PRB");
      return -1;
    }
    d.sf = (uint32_t)s;
    d.dup = (s + 1 < n && !owns[s + 1]) ? (uint32_t)(s + 1) : 0xFFFFFFFFu;   // a pair: cw 0 then cw 1
    sfs.push_back(d);
  }
  return 0;
}

bool CsiEngine::matches(const Plan& P) const {
  if (P.sfs.size() != ce_off.size() || P.ce_elems != ce_elems) return false;
  for (size_t s = 0; s < ce_off.size(); s++)
    if (P.sfs[s].ce_off != ce_off[s]) return false;
  for (const MiCsiSf& d : sfs) {
    const MiCellDesc& c = P.cells[P.sfs[d.sf].cell];
    if (c.W != d.W || c.nof_ports != d.ports) return false;
  }
  return true;
}

int CsiEngine::upload() {
  const size_t n = ce_off.size();
  const bool ok = d_sfs.ensure(sfs.size() * sizeof(MiCsiSf)) && d_out.ensure(n * sizeof(mi_dl_csi_result_t)) &&
                  d_noise.ensure(n * sizeof(float)) &&
                  hip_ok(hipMemcpy(d_sfs.p, sfs.data(), sfs.size() * sizeof(MiCsiSf), hipMemcpyHostToDevice), "H2D") &&
                  hip_ok(hipMemset(d_out.p, 0, n * sizeof(mi_dl_csi_result_t)), "memset");
  return ok ? 0 : -1;
}

}  // namespace mi

// ---- C ABI (include/mi_dl.h) -----------------------------------------------------------------
struct mi_dl_csi {
  mi::CsiEngine eng;
  mi_dl_batch_t* b = nullptr;
  hipStream_t last = nullptr;
  bool own_noise = false;   // set_noise gave values: d_noise replaces the chest metrics
  bool have = false;        // `res` holds the last run's records
  std::vector<mi_dl_csi_result_t> res;
};

static int csi_fetch(mi_dl_csi_t* c) {
  if (c->have) return 0;
  c->res.resize(c->eng.ce_off.size());
  if (!mi::hip_ok(hipStreamSynchronize(c->last), "sync") ||
      !mi::hip_ok(hipMemcpy(c->res.data(), c->eng.d_out.p, c->res.size() * sizeof(mi_dl_csi_result_t),
                            hipMemcpyDeviceToHost), "D2H"))
    return -1;
  c->have = true;
  return 0;
}

extern "C" {

mi_dl_csi_t* mi_dl_csi_create(mi_dl_batch_t* b) {
  if (!b) { mi::set_error("null batch"); return nullptr; }
  auto* c = new mi_dl_csi();
  c->b = b;
  if (c->eng.build(b->eng.plan) || c->eng.upload()) { delete c; return nullptr; }
  return c;
}

void mi_dl_csi_destroy(mi_dl_csi_t* c) { delete c; }

uint32_t mi_dl_csi_n(const mi_dl_csi_t* c) { return c ? (uint32_t)c->eng.ce_off.size() : 0; }

int mi_dl_csi_set_noise(mi_dl_csi_t* c, const float* per_sf) {
  if (!c) { mi::set_error("null argument"); return -1; }
  if (!per_sf) { c->own_noise = false; return 0; }
  // a queued run may still read the previous values
  if (!mi::hip_ok(hipStreamSynchronize(c->last), "sync") ||
      !mi::hip_ok(hipMemcpy(c->eng.d_noise.p, per_sf, c->eng.ce_off.size() * sizeof(float), hipMemcpyHostToDevice), "H2D"))
    return -1;
  c->own_noise = true;
  return 0;
}

int mi_dl_csi_run(mi_dl_csi_t* c, void* stream) {
  if (!c) { mi::set_error("null argument"); return -1; }
  const mi::Engine& e = c->b->eng;
  if (!c->eng.matches(e.plan)) {
    mi::set_error("mi_dl_csi_run: the batch was re-planned since mi_dl_csi_create: create a new object");
    return -1;
  }
  if (!e.ce_written || (!c->own_noise && !e.metrics_written)) {
    mi::set_error("mi_dl_csi_run: no channel estimates yet: run the batch with the CHEST stage first");
    return -1;
  }
  c->last = reinterpret_cast<hipStream_t>(stream);
  c->have = false;
  const mi::RxPlanes rx{e.n_rx, e.plan.iq_samples, e.plan.grid_elems, e.plan.ce_elems};
  mi::launch_csi(e.d_ce.as<float2>(), e.d_metrics.as<float>(), c->own_noise ? c->eng.d_noise.as<float>() : nullptr,
                 c->eng.d_sfs.as<MiCsiSf>(), (uint32_t)c->eng.sfs.size(), c->eng.d_out.as<mi_dl_csi_result_t>(),
                 e.ce_compact, rx, (uint32_t)c->eng.ce_off.size(), c->last);
  return mi::hip_ok(hipGetLastError(), "csi launch") ? 0 : -1;
}

int mi_dl_csi_result(mi_dl_csi_t* c, uint32_t sf, mi_dl_csi_result_t* out) {
  if (!c || !out || sf >= c->eng.ce_off.size()) { mi::set_error("mi_dl_csi_result: bad subframe or null argument"); return -1; }
  if (csi_fetch(c)) return -1;
  *out = c->res[sf];
  return 0;
}

int mi_dl_csi_download(mi_dl_csi_t* c, mi_dl_csi_result_t* out) {
  if (!c || !out) { mi::set_error("null argument"); return -1; }
  if (csi_fetch(c)) return -1;
  memcpy(out, c->res.data(), c->res.size() * sizeof(mi_dl_csi_result_t));
  return 0;
}

void* mi_dl_csi_device_ptr(mi_dl_csi_t* c) { return c ? c->eng.d_out.p : nullptr; }

int mi_csi_subbands(uint32_t nof_prb, uint32_t* sb_prb, uint32_t* n_sb) {
  uint32_t k = 0, n = 0;
  if (!mi::csi_subbands(nof_prb, &k, &n)) { mi::set_error("mi_csi_subbands: nof_prb outside 6..110"); return -1; }
  if (sb_prb) *sb_prb = k;
  if (n_sb) *n_sb = n;
  return 0;
}

int mi_csi_pack_pucch(uint32_t tm, const mi_dl_csi_result_t* r, uint8_t bits[11], uint32_t* ri) {
  if (!r || !bits || tm < 1 || tm > 4) { mi::set_error("mi_csi_pack_pucch: tm 1..4, record and bits"); return -1; }
  uint32_t n = 0, rank = 1;
  auto put = [&](uint32_t v, uint32_t w) {   // MSB first
    for (uint32_t i = 0; i < w; i++) bits[n++] = (uint8_t)((v >> (w - 1 - i)) & 1u);
  };
  auto has = [&](uint32_t h) { return ((r->valid_mask >> h) & 1u) != 0; };
  if (tm <= 3) {
    uint32_t h = MI_CSI_H_BASE;
    if (tm == 3 && r->ri_ol == 2) { h = MI_CSI_H_CDD; rank = 2; }
    if (!has(h)) { mi::set_error("mi_csi_pack_pucch: hypothesis not evaluated"); return -1; }
    put(r->cqi[0][h][0], 4);
  } else if (r->ri_cl == 2) {
    if (r->cb_r2 < 1 || r->cb_r2 > 2 || !has(MI_CSI_H_R2 + r->cb_r2 - 1)) {
      mi::set_error("mi_csi_pack_pucch: rank-2 hypotheses not evaluated");
      return -1;
    }
    const uint8_t* q = r->cqi[0][MI_CSI_H_R2 + r->cb_r2 - 1];
    const int off = (int)q[0] - (int)q[1];   // 36.213 Table 7.2-2
    rank = 2;
    put(q[0], 4);
    put(off >= 3 ? 3u : off >= 0 ? (uint32_t)off : off <= -4 ? 4u : (uint32_t)(8 + off), 3);
    put(r->cb_r2 - 1, 1);
  } else {
    if (r->pmi_r1 > 3 || !has(MI_CSI_H_R1 + r->pmi_r1)) {
      mi::set_error("mi_csi_pack_pucch: rank-1 hypotheses not evaluated (one CRS port)");
      return -1;
    }
    put(r->cqi[0][MI_CSI_H_R1 + r->pmi_r1][0], 4);
    put(r->pmi_r1, 2);
  }
  if (ri) *ri = rank;
  return (int)n;
}

}  // extern "C"
