// pucch_host.cpp -- host planner of the PUCCH transmitter (see pucch.h; no HIP calls).  Spec arithmetic:
// 36.211 5.4.1 / 5.4.2 (resource to n', orthogonal cover, cyclic shift), 5.4.3 (PRB mapping), 5.5.1.3 (group
// hopping), 36.213 10.1 (format and resource selection, FDD).  DESIGN.md carries the formulas as implemented.
#include "pucch.h"

#include <string.h>

#include "plan.h"     // set_error
#include "tables.h"   // gold_bits
#include "ul_plan.h"  // ul_cqi_code, ul_group_u

namespace mi {
namespace {

constexpr uint32_t C_NORM = 3, D_NORM = 2, NSC = 12;   // c and d of 5.4.1 for the normal CP, N_sc^RB

// what depends on the cell alone: n_cs^cell(ns, l) of every slot of the frame
struct CellSeq {
  uint32_t cell_id = 0xFFFFFFFFu;
  uint8_t ncs[20][7];
  void load(uint32_t id) {
    if (id == cell_id) return;
    std::vector<uint8_t> c(8 * 7 * 20);
    gold_bits(id, (uint32_t)c.size(), c.data());        // 5.4: c_init = N_ID^cell
    for (uint32_t ns = 0; ns < 20; ns++)
      for (uint32_t l = 0; l < 7; l++) {
        uint32_t v = 0;
        for (uint32_t i = 0; i < 8; i++) v += (uint32_t)c[8 * 7 * ns + 8 * l + i] << i;
        ncs[ns][l] = (uint8_t)(v % NSC);   // only n_cs^cell mod 12 enters n_cs
      }
    cell_id = id;
  }
};

bool is_f2(uint32_t format) { return format >= MI_PUCCH_2; }

// every field of c, and the resource block index m (5.4.3) it leads to; false + set_error
bool check(const mi_pucch_cfg_t& c, uint32_t* m_out) {
  if (!std_nof_prb(c.nof_prb)) {
    set_error("PUCCH: nof_prb must be one of 6, 15, 25, 50, 75, 100");
    return false;
  }
  if (c.cell_id > 503 || c.sf_idx > 9 || c.rnti > 0xFFFFu || c.format > MI_PUCCH_2B) {
    set_error("PUCCH: cell_id 0..503, sf_idx 0..9, 16-bit RNTI, format MI_PUCCH_1 .. MI_PUCCH_2B");
    return false;
  }
  if (c.delta_shift < 1 || c.delta_shift > 3) {
    set_error("PUCCH: deltaPUCCH-Shift must be 1, 2 or 3");
    return false;
  }
  if (c.N_cs > 7 || c.N_cs % c.delta_shift) {
    set_error("PUCCH: nCS-AN must be 0..7 and a multiple of deltaPUCCH-Shift");
    return false;
  }
  uint32_t m;
  if (is_f2(c.format)) {
    if (c.shortened) {
      set_error("PUCCH: the shortened format exists for formats 1/1a/1b only");
      return false;
    }
    if (c.cqi_len < 1 || c.cqi_len > (uint32_t)PUCCH_NCOL) {
      set_error("PUCCH: formats 2/2a/2b carry A = 1..11 CQI bits");
      return false;
    }
    m = c.n_pucch / NSC;
  } else {
    const uint32_t T = C_NORM * c.N_cs / c.delta_shift, per = C_NORM * NSC / c.delta_shift;
    m = c.n_pucch < T ? c.n_rb_2 : (c.n_pucch - T) / per + c.n_rb_2 + (c.N_cs + 7) / 8;
  }
  if (c.n_rb_2 >= c.nof_prb || m >= c.nof_prb) {
    set_error("PUCCH: the resource maps outside the cell (m >= nof_prb)");
    return false;
  }
  *m_out = m;
  return true;
}

void derive(const mi_pucch_cfg_t& c, uint32_t m, CellSeq& cs, mi_pucch_res_t* r) {
  cs.load(c.cell_id);
  const uint32_t D = c.delta_shift;
  uint32_t np[2], Np = NSC;
  if (is_f2(c.format)) {
    const bool own = c.n_pucch < NSC * c.n_rb_2;   // in a format-2 RB (else the mixed RB)
    np[0] = own ? c.n_pucch % NSC : (c.n_pucch + c.N_cs + 1) % NSC;
    np[1] = own ? (NSC * (np[0] + 1)) % (NSC + 1) - 1 : (NSC - 2 + NSC - c.n_pucch % NSC) % NSC;
  } else {
    const uint32_t T = C_NORM * c.N_cs / D, per = C_NORM * NSC / D;
    const bool mixed = c.n_pucch < T;
    Np = mixed ? c.N_cs : NSC;
    np[0] = mixed ? c.n_pucch : (c.n_pucch - T) % per;
    if (mixed) {
      const uint32_t h = (np[0] + D_NORM) % (C_NORM * Np / D);
      np[1] = h / C_NORM + (h % C_NORM) * Np / D;
    } else {
      np[1] = (C_NORM * (np[0] + 1)) % (per + 1) - 1;   // per + 1 is 37, 19 or 13: the residue is never 0
    }
  }
  for (uint32_t s = 0; s < 2; s++) {
    const uint32_t ns = 2 * c.sf_idx + s;
    r->n_prb[s] = (m + s) % 2 == 0 ? m / 2 : c.nof_prb - 1 - m / 2;
    r->u[s] = ul_group_u(c.cell_id, ns, c.group_hopping, c.cell_id % 30);
    r->n_prime[s] = np[s];
    r->n_oc[s] = is_f2(c.format) ? 0 : np[s] * D / Np;
    const uint32_t off = is_f2(c.format) ? np[s] : (np[s] * D + r->n_oc[s] % D) % Np;
    for (uint32_t l = 0; l < 7; l++) r->n_cs[s][l] = (cs.ncs[ns][l] + off) % NSC;
  }
}

// srsUE's workers stay on one cell: the sequences are derived once per thread and cell
thread_local CellSeq g_cell;

}  // namespace

int PucchPlan::build(const mi_pucch_cfg_t* cfgs, uint32_t n) {
  txs.clear();
  res.clear();
  iq_samples = 0;
  std::vector<uint32_t> ms(n);
  for (uint32_t i = 0; i < n; i++)
    if (!check(cfgs[i], &ms[i])) return -1;
  // the (20, A) code (36.212 5.2.3.3) by columns: rows 0..19 of the (32, O) basis ul_plan.cpp holds, derived once
  static const std::vector<uint32_t> cols = [] {
    std::vector<uint32_t> v(PUCCH_NCOL, 0u);
    for (uint32_t k = 0; k < (uint32_t)PUCCH_NCOL; k++) {
      uint8_t o[PUCCH_NCOL] = {};
      o[k] = 1;
      std::vector<uint8_t> q;
      ul_cqi_code(o, PUCCH_NCOL, 32, q);
      for (uint32_t i = 0; i < 20; i++) v[k] |= (uint32_t)q[i] << (31 - i);
    }
    return v;
  }();
  memcpy(rm, cols.data(), sizeof(rm));
  for (uint32_t i = 0; i < n; i++) {
    const mi_pucch_cfg_t& c = cfgs[i];
    mi_pucch_res_t r;
    derive(c, ms[i], g_cell, &r);
    MiPucchTx t{};
    t.N = (uint32_t)symbol_sz(c.nof_prb);
    t.W = 12 * c.nof_prb;
    t.format = c.format;
    t.shortened = c.shortened ? 1 : 0;
    t.cqi_len = is_f2(c.format) ? c.cqi_len : 0;
    t.scale = 1.0f;
    t.cfo = 0.0f;
    for (uint32_t s = 0; s < 2; s++) {
      t.n_prb[s] = r.n_prb[s];
      t.u[s] = r.u[s];
      t.n_oc[s] = r.n_oc[s];
      t.s_odd[s] = r.n_prime[s] & 1u;
      for (uint32_t l = 0; l < 7; l++) t.ncs[s] |= r.n_cs[s][l] << (4 * l);
    }
    if (is_f2(c.format)) {   // 5.4.2: c_init = (floor(ns / 2) + 1) (2 N_ID + 1) 2^16 + n_RNTI
      uint8_t b[20];
      gold_bits((c.sf_idx + 1) * (2 * c.cell_id + 1) * 65536u + c.rnti, 20, b);
      for (uint32_t k = 0; k < 20; k++) t.scr |= (uint32_t)b[k] << (31 - k);
    }
    t.iq_off = iq_samples;
    iq_samples += 15 * (size_t)t.N;
    txs.push_back(t);
    res.push_back(r);
  }
  return 0;
}

}  // namespace mi

extern "C" {

uint32_t mi_pucch_resource_n(const mi_pucch_cfg_t* c, uint32_t n, mi_pucch_res_t* r) {
  if (!c || !r) { mi::set_error("PUCCH: null argument"); return 0; }
  for (uint32_t i = 0; i < n; i++) {
    uint32_t m;
    if (!mi::check(c[i], &m)) return i;
    mi::derive(c[i], m, mi::g_cell, &r[i]);
  }
  return n;
}

int mi_pucch_resource(const mi_pucch_cfg_t* c, mi_pucch_res_t* r) { return mi_pucch_resource_n(c, 1, r) == 1 ? 0 : -1; }

int mi_pucch_select(uint32_t ack_len, int sr, uint32_t cqi_len, int simul_cqi_ack_dropped, uint32_t n_cce,
                    uint32_t N_pucch_1, uint32_t n_pucch_2, uint32_t n_pucch_sr, uint32_t* n_pucch) {
  if (ack_len > 2) ack_len = 2;
  uint32_t res;
  int format;
  if (sr) {   // a positive SR: HARQ-ACK (if any) on the SR resource, a CQI is dropped
    format = ack_len == 0 ? MI_PUCCH_1 : ack_len == 1 ? MI_PUCCH_1A : MI_PUCCH_1B;
    res = n_pucch_sr;
  } else if (cqi_len && !(ack_len && simul_cqi_ack_dropped)) {
    format = ack_len == 0 ? MI_PUCCH_2 : ack_len == 1 ? MI_PUCCH_2A : MI_PUCCH_2B;
    res = n_pucch_2;
  } else if (ack_len) {
    format = ack_len == 1 ? MI_PUCCH_1A : MI_PUCCH_1B;
    res = n_cce + N_pucch_1;
  } else {
    return -1;
  }
  if (n_pucch) *n_pucch = res;
  return format;
}

}  // extern "C"
