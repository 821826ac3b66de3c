// dci2_host.cpp -- DCI formats 2 / 2A (36.212 5.3.3.1.5 / 5.3.3.1.5A, FDD, 2 CRS ports): size, pack, unpack and the
// batch entries that decode an unpacked grant (include/mi_dl.h mi_dci_dl2_*).  Host only: no HIP call.
#include <string.h>

#include "dl_common.h"
#include "mi_dl.h"
#include "plan.h"
#include "tables.h"

namespace {

// the field widths of one (format, bandwidth): everything pack and unpack walk
struct Dci2Layout {
  uint32_t P, nrbg, hdr, pb, nt1, pinfo_bits, size;
};

bool dci2_layout(uint32_t format, uint32_t nof_prb, uint32_t nof_ports, Dci2Layout* l) {
  if (format != MI_DCI_2 && format != MI_DCI_2A) { mi::set_error("dci2: format"); return false; }
  if (nof_ports != 2) { mi::set_error("dci2: formats 2 / 2A are built for 2 CRS ports"); return false; }
  if (nof_prb < 6 || nof_prb > MI_DL_MAX_PRB) { mi::set_error("dci2: nof_prb"); return false; }
  l->P = mi::rbg_size(nof_prb);
  l->nrbg = (nof_prb + l->P - 1) / l->P;
  l->hdr = nof_prb > 10 ? 1 : 0;
  l->pb = mi::ceil_log2(l->P);
  l->nt1 = l->hdr ? l->nrbg - l->pb - 1 : 0;
  l->pinfo_bits = format == MI_DCI_2 ? 3 : 0;
  l->size = mi::dci_size((int)format, nof_prb);
  return true;
}

void put_bits(uint8_t* b, uint32_t* pos, uint32_t v, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) b[(*pos)++] = (uint8_t)((v >> (n - 1 - i)) & 1u);
}
uint32_t get_bits(const uint8_t* b, uint32_t* pos, uint32_t n) {
  uint32_t v = 0;
  for (uint32_t i = 0; i < n; i++) v = (v << 1) | (b[(*pos)++] & 1u);
  return v;
}
bool fits(uint32_t v, uint32_t n) { return n >= 32 || v < (1u << n); }

}  // namespace

extern "C" {

int mi_dci_dl2_size(uint32_t format, uint32_t nof_prb, uint32_t nof_ports) {
  Dci2Layout l;
  return dci2_layout(format, nof_prb, nof_ports, &l) ? (int)l.size : -1;
}

int mi_dci_dl2_pack(uint32_t nof_prb, uint32_t nof_ports, const mi_dci_dl2_t* d, uint8_t bits[64]) {
  Dci2Layout l;
  if (!d || !bits) { mi::set_error("null argument"); return -1; }
  if (!dci2_layout(d->format, nof_prb, nof_ports, &l)) return -1;
  bool ok = d->alloc_type <= l.hdr && fits(d->tpc_pucch, 2) && fits(d->harq_process, 3) && fits(d->tb_cw_swap, 1) &&
            fits(d->pinfo, l.pinfo_bits);
  if (d->alloc_type == 0) ok = ok && fits(d->type0_alloc, l.nrbg);
  else ok = ok && d->type1_subset < l.P && fits(d->type1_shift, 1) && fits(d->type1_bitmap, l.nt1);
  for (int t = 0; t < 2; t++)
    ok = ok && fits(d->tb[t].mcs, 5) && fits(d->tb[t].ndi, 1) && fits(d->tb[t].rv, 2) &&
         d->tb[t].enabled == (uint32_t)!(d->tb[t].mcs == 0 && d->tb[t].rv == 1);
  if (!ok) { mi::set_error("dci2: field out of range"); return -1; }
  uint32_t pos = 0;
  memset(bits, 0, 64);
  if (l.hdr) put_bits(bits, &pos, d->alloc_type, 1);
  if (d->alloc_type == 0) {
    put_bits(bits, &pos, d->type0_alloc, l.nrbg);
  } else {
    put_bits(bits, &pos, d->type1_subset, l.pb);
    put_bits(bits, &pos, d->type1_shift, 1);
    put_bits(bits, &pos, d->type1_bitmap, l.nt1);
  }
  put_bits(bits, &pos, d->tpc_pucch, 2);
  put_bits(bits, &pos, d->harq_process, 3);
  put_bits(bits, &pos, d->tb_cw_swap, 1);
  for (int t = 0; t < 2; t++) {
    put_bits(bits, &pos, d->tb[t].mcs, 5);
    put_bits(bits, &pos, d->tb[t].ndi, 1);
    put_bits(bits, &pos, d->tb[t].rv, 2);
  }
  put_bits(bits, &pos, d->pinfo, l.pinfo_bits);
  return (int)l.size;   // pos, or pos + 1: the appended zero bit
}

int mi_dci_dl2_unpack(uint32_t format, uint32_t nof_prb, uint32_t nof_ports, const uint8_t* bits, uint32_t nbits,
                      mi_dci_dl2_t* d) {
  Dci2Layout l;
  if (!d || !bits) { mi::set_error("null argument"); return -1; }
  if (!dci2_layout(format, nof_prb, nof_ports, &l)) return -1;
  if (nbits != l.size) { mi::set_error("dci2: payload size"); return -1; }
  mi_dci_dl2_t o;
  memset(&o, 0, sizeof(o));
  o.format = format;
  uint32_t pos = 0;
  o.alloc_type = l.hdr ? get_bits(bits, &pos, 1) : 0;
  if (o.alloc_type == 0) {
    o.type0_alloc = get_bits(bits, &pos, l.nrbg);
  } else {
    o.type1_subset = get_bits(bits, &pos, l.pb);
    o.type1_shift = get_bits(bits, &pos, 1);
    o.type1_bitmap = get_bits(bits, &pos, l.nt1);
    if (o.type1_subset >= l.P) { mi::set_error("dci2: type 1 subset"); return -1; }
  }
  o.tpc_pucch = get_bits(bits, &pos, 2);
  o.harq_process = get_bits(bits, &pos, 3);
  o.tb_cw_swap = get_bits(bits, &pos, 1);
  for (int t = 0; t < 2; t++) {
    o.tb[t].mcs = get_bits(bits, &pos, 5);
    o.tb[t].ndi = get_bits(bits, &pos, 1);
    o.tb[t].rv = get_bits(bits, &pos, 2);
    o.tb[t].enabled = !(o.tb[t].mcs == 0 && o.tb[t].rv == 1);
  }
  o.pinfo = get_bits(bits, &pos, l.pinfo_bits);
  *d = o;
  return 0;
}

int mi_dci_dl2_to_cfg(const mi_dci_dl2_t* d, const mi_dl_sf_cfg_t* base, const uint8_t new_tb[2],
                      uint32_t reported_cb_r2, mi_dl_sf_cfg_t out[2]) {
  Dci2Layout l;
  if (!d || !base || !new_tb || !out) { mi::set_error("null argument"); return -1; }
  if (!dci2_layout(d->format, base->nof_prb, base->nof_ports, &l)) return -1;
  if (d->alloc_type > l.hdr) { mi::set_error("dci2: allocation type"); return -1; }
  uint8_t prb[MI_DL_MAX_PRB];
  const int n_prb = mi::ra_type01_prbs(base->nof_prb, d->alloc_type == 1, d->type0_alloc, d->type1_subset,
                                       d->type1_shift, d->type1_bitmap, prb);
  if (n_prb <= 0) { mi::set_error("dci2: resource allocation"); return -1; }
  const bool en[2] = {!(d->tb[0].mcs == 0 && d->tb[0].rv == 1), !(d->tb[1].mcs == 0 && d->tb[1].rv == 1)};
  if (!en[0] && !en[1]) { mi::set_error("dci2: both transport blocks disabled"); return -1; }
  const bool pair = en[0] && en[1];
  uint32_t tm = 2, pmi = 0;
  if (pair) {
    tm = d->format == MI_DCI_2A ? 3 : 4;
    if (d->format == MI_DCI_2) {   // 36.212 Table 5.3.3.1.5-4, two codewords
      pmi = d->pinfo == 0 ? 1 : d->pinfo == 1 ? 2 : d->pinfo == 2 ? reported_cb_r2 : 0;
      if (d->pinfo > 2) { mi::set_error("dci2: reserved precoding information"); return -1; }
      if (pmi != 1 && pmi != 2) { mi::set_error("dci2: no rank-2 codebook index reported"); return -1; }
    }
  } else if (d->format == MI_DCI_2 && d->pinfo != 0) {   // one codeword: 0 = transmit diversity
    mi::set_error(d->pinfo <= 6 ? "dci2: rank-1 precoding is not built" : "dci2: reserved precoding information");
    return -1;
  }
  // transport block of each codeword (Tables 5.3.3.1.5-1 / -2)
  const int tb_of_cw[2] = {pair ? (d->tb_cw_swap ? 1 : 0) : (en[0] ? 0 : 1), pair ? (d->tb_cw_swap ? 0 : 1) : -1};
  mi_dl_sf_cfg_t tmp[2];
  const int n_out = pair ? 2 : 1;
  for (int q = 0; q < n_out; q++) {
    const int t = tb_of_cw[q];
    uint32_t qm = 0;
    const int itbs = mi::mcs_to_itbs(d->tb[t].mcs, &qm);   // MCS 29..31 (TBS from the previous grant): -1
    const int tbs = itbs < 0 ? -1 : mi::tbs_from_idx((uint32_t)itbs, (uint32_t)n_prb);
    if (tbs <= 0) { mi::set_error("dci2: MCS 29..31 is not built"); return -1; }
    mi_dl_sf_cfg_t& c = tmp[q];
    memset(&c, 0, sizeof(c));
    c.cell_id = base->cell_id;
    c.nof_prb = base->nof_prb;
    c.nof_ports = base->nof_ports;
    c.sf_idx = base->sf_idx;
    c.cfi = base->cfi;
    c.rnti = base->rnti;
    c.tm = tm;
    c.nl_td = 2;
    c.rv = d->tb[t].rv;
    c.tbs = (uint32_t)tbs;
    c.Qm = qm;
    c.new_tb = new_tb[t] ? 1 : 0;
    memcpy(c.prb_mask, prb, base->nof_prb);
    c.cw = (uint32_t)q;
    c.pmi = pmi;
  }
  memcpy(out, tmp, sizeof(mi_dl_sf_cfg_t) * (size_t)n_out);
  return n_out;
}

}  // extern "C"
