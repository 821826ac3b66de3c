// pbch_host.cpp -- host planner of the PBCH receiver (pbch.h) and the mi_pbch_* C ABI.
#include <string.h>

#include <map>

#include "batch_impl.h"
#include "kernels.h"
#include "pbch.h"
#include "tables.h"

namespace mi {

// 36.211 6.6.4: the 72 centre subcarriers of symbols 0..3 of slot 1, symbol then subcarrier, without the REs
// reserved for CRS of antenna ports 0-3 (symbols 7 and 8: k mod 3 = N_ID mod 3) whatever the cell's port count
void pbch_re_list(uint32_t cell_id, uint32_t nof_prb, uint32_t* re) {
  const uint32_t W = 12 * nof_prb, k0 = 6 * nof_prb - 36;
  uint32_t n = 0;
  for (uint32_t l = 7; l <= 10; l++)
    for (uint32_t k = k0; k < k0 + 72; k++) {
      if (l <= 8 && k % 3 == cell_id % 3) continue;
      re[n++] = l * W + k;
    }
}

int PbchEngine::build(const Plan& P) {
  frames.clear(); frame_cell.clear(); frame_scr.clear(); cdata.clear(); jobs.clear(); job_begin.assign(1, 0);
  frame_of_sf.assign(P.sfs.size(), -1);
  std::vector<uint32_t> rank;
  conv_rank_table(PBCH_D, rank);
  rank_off = 0;
  cdata.insert(cdata.end(), rank.begin(), rank.end());
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> re_cache;   // (id mod 3, nof_prb) -> cdata offset
  std::map<uint32_t, uint32_t> scr_cache;                        // id -> cdata offset
  for (size_t s = 0; s < P.sfs.size(); s++) {
    const MiSfDesc& sd = P.sfs[s];
    if (sd.sf_idx != 0) continue;
    const MiCellDesc& c = P.cells[sd.cell];
    MiPbchFrame d{};
    d.grid_off = sd.grid_off;
    d.ce_off = sd.ce_off;
    d.plane = NSYMB * c.W;
    d.ports = c.nof_ports;
    auto ri = re_cache.find({c.id % 3, c.nof_prb});
    if (ri == re_cache.end()) {
      uint32_t re[PBCH_RE];
      pbch_re_list(c.id, c.nof_prb, re);
      ri = re_cache.emplace(std::make_pair(c.id % 3, c.nof_prb), (uint32_t)cdata.size()).first;
      cdata.insert(cdata.end(), re, re + PBCH_RE);
    }
    d.re_off = ri->second;
    auto si = scr_cache.find(c.id);
    if (si == scr_cache.end()) {
      uint32_t w[PBCH_E / 32];
      gold_words(c.id, PBCH_E, w);   // 36.211 6.6.1: c_init = N_ID^cell at the start of each BCH TTI
      si = scr_cache.emplace(c.id, (uint32_t)cdata.size()).first;
      cdata.insert(cdata.end(), w, w + PBCH_E / 32);
    }
    frame_of_sf[s] = (int32_t)frames.size();
    frames.push_back(d);
    frame_cell.push_back(sd.cell);
    frame_scr.push_back(si->second);
  }
  return 0;
}

template <class T>
static bool up_vec(DevBuf& b, const std::vector<T>& v, hipStream_t st) {
  return b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T)) &&
         (v.empty() || hip_ok(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st), "H2D"));
}

int PbchEngine::upload(hipStream_t st) {
  const bool ok = up_vec(d_frames, frames, st) && up_vec(d_cdata, cdata, st) &&
                  d_llr.ensure(std::max<size_t>(llr_floats(), 1) * 4) && hip_ok(hipStreamSynchronize(st), "pbch upload");
  return ok ? 0 : -1;
}

int PbchEngine::set_candidates(const Plan& P, const uint32_t* sf, const uint32_t* n_frames, uint32_t n_cand,
                               hipStream_t st) {
  jobs.clear(); job_ports.clear(); job_f.clear(); job_phase.clear(); job_begin.assign(1, 0);
  // every check first: nothing below indexes with a value that was not checked here
  for (uint32_t c = 0; c < n_cand; c++) {
    if (n_frames[c] < 1 || n_frames[c] > 4) { set_error("pbch: a candidate has 1..4 frames"); return -1; }
    for (uint32_t i = 0; i < n_frames[c]; i++) {
      const uint32_t s = sf[4 * c + i];
      if (s >= frame_of_sf.size()) { set_error("pbch: candidate frame outside the batch"); return -1; }
      if (frame_of_sf[s] < 0) { set_error("pbch: candidate frame is not a subframe 0"); return -1; }
      if (frame_cell[(size_t)frame_of_sf[s]] != frame_cell[(size_t)frame_of_sf[sf[4 * c]]]) {
        set_error("pbch: candidate frames of different cells");
        return -1;
      }
    }
  }
  for (uint32_t c = 0; c < n_cand; c++) {
    const uint32_t n = n_frames[c];
    const uint32_t fr0 = (uint32_t)frame_of_sf[sf[4 * c]];
    const uint32_t ports = P.cells[frame_cell[fr0]].nof_ports;
    // search order: frames combined ascending, then 1 port before 2, then the phase of the newest frame
    for (uint32_t f = 1; f <= n; f++)
      for (uint32_t np = 1; np <= (ports == 2 ? 2u : 1u); np++)
        for (uint32_t phi = f - 1; phi <= 3; phi++) {
          MiPbchJob j{};
          for (uint32_t i = 0; i < f; i++) {
            const uint32_t fr = (uint32_t)frame_of_sf[sf[4 * c + (n - f) + i]];
            j.llr_off[i] = (fr * 2 + (np - 1)) * PBCH_BITS;
          }
          j.f = f;
          j.phase0 = phi - (f - 1);
          j.scr_off = frame_scr[fr0];
          j.mask = np == 1 ? 0x0000u : 0xFFFFu;
          jobs.push_back(j);
          job_ports.push_back((uint8_t)np);
          job_f.push_back((uint8_t)f);
          job_phase.push_back((uint8_t)phi);
        }
    job_begin.push_back((uint32_t)jobs.size());
  }
  res.clear();
  const bool ok = up_vec(d_jobs, jobs, st) && d_res.ensure(std::max<size_t>(jobs.size(), 1) * sizeof(MiPbchRes)) &&
                  hip_ok(hipStreamSynchronize(st), "pbch candidates");
  return ok ? 0 : -1;
}

int PbchEngine::run(const float2* grid, const float2* ce, uint32_t mask, float noise, hipStream_t st) {
  if (mask & 1u)
    launch_pbch_llr(grid, ce, d_frames.as<MiPbchFrame>(), d_cdata.as<uint32_t>(), d_llr.as<float>(),
                    (uint32_t)frames.size(), noise, st);
  if (mask & 2u)
    launch_pbch_decode(d_llr.as<float>(), d_jobs.as<MiPbchJob>(), d_cdata.as<uint32_t>(), rank_off, d_res.as<MiPbchRes>(),
                       (uint32_t)jobs.size(), st);
  return hip_ok(hipGetLastError(), "pbch launch") ? 0 : -1;
}

int PbchEngine::download(hipStream_t st) {
  res.resize(jobs.size());
  if (res.empty()) return hip_ok(hipStreamSynchronize(st), "sync") ? 0 : -1;
  return hip_ok(hipMemcpyAsync(res.data(), d_res.p, res.size() * sizeof(MiPbchRes), hipMemcpyDeviceToHost, st), "D2H") &&
                 hip_ok(hipStreamSynchronize(st), "sync")
             ? 0
             : -1;
}

PbchFound PbchEngine::select(uint32_t cand) const {
  PbchFound out{};
  for (uint32_t j = job_begin[cand]; j < job_begin[cand + 1]; j++) {
    if (!res[j].found) continue;
    out.found = 1;
    out.nof_ports = job_ports[j];
    out.sfn_offset = job_phase[j];
    out.n_frames_used = job_f[j];
    for (uint32_t i = 0; i < PBCH_A; i++) out.bits[i] = (uint8_t)((res[j].bits >> (PBCH_A - 1 - i)) & 1u);
    return out;
  }
  return out;
}

}  // namespace mi

// ---- C ABI (include/mi_dl.h) -----------------------------------------------------------------
struct mi_pbch {
  mi::PbchEngine pe;
  mi_dl_batch_t* b = nullptr;
  hipStream_t last = nullptr;
  bool have_res = false;
};

extern "C" {

int mi_pbch_re_indices(uint32_t cell_id, uint32_t nof_prb, uint32_t re[240]) {
  if (!re || cell_id > 503 || nof_prb < 6 || mi::symbol_sz(nof_prb) < 0) { mi::set_error("mi_pbch_re_indices: arguments"); return -1; }
  mi::pbch_re_list(cell_id, nof_prb, re);
  return 0;
}

mi_pbch_t* mi_pbch_create(mi_dl_batch_t* b) {
  if (!b) { mi::set_error("null batch"); return nullptr; }
  auto* p = new mi_pbch();
  p->b = b;
  if (p->pe.build(b->eng.plan) || p->pe.upload(nullptr)) { delete p; return nullptr; }
  return p;
}

void mi_pbch_destroy(mi_pbch_t* p) { delete p; }

uint32_t mi_pbch_n_frames(const mi_pbch_t* p) { return p ? (uint32_t)p->pe.frames.size() : 0; }
uint32_t mi_pbch_n_jobs(const mi_pbch_t* p) { return p ? (uint32_t)p->pe.jobs.size() : 0; }
int mi_pbch_frame_of(const mi_pbch_t* p, uint32_t sf) {
  return (p && sf < p->pe.frame_of_sf.size()) ? p->pe.frame_of_sf[sf] : -1;
}

int mi_pbch_set_candidates(mi_pbch_t* p, const uint32_t* sf, const uint32_t* n_frames, uint32_t n_cand) {
  if (!p || (n_cand && (!sf || !n_frames))) { mi::set_error("null argument"); return -1; }
  if (p->last && !mi::hip_ok(hipStreamSynchronize(p->last), "sync")) return -1;   // a run may still read the old jobs
  p->have_res = false;
  return p->pe.set_candidates(p->b->eng.plan, sf, n_frames, n_cand, p->last);
}

int mi_pbch_run(mi_pbch_t* p, uint32_t mask, void* stream) {
  if (!p) { mi::set_error("null argument"); return -1; }
  if ((mask & 1u) && p->b->eng.ce_compact) { mi::set_error("pbch: the batch holds compact channel estimates"); return -1; }
  p->last = reinterpret_cast<hipStream_t>(stream);
  p->have_res = false;
  return p->pe.run(p->b->eng.d_grid.as<float2>(), p->b->eng.d_ce.as<float2>(), mask, 0.0f, p->last);
}

int mi_pbch_result(mi_pbch_t* p, uint32_t cand, mi_pbch_result_t* out) {
  if (!p || cand + 1 >= p->pe.job_begin.size()) { mi::set_error("bad candidate"); return -1; }
  if (!p->have_res) {
    if (p->pe.download(p->last)) return -1;
    p->have_res = true;
  }
  const mi::PbchFound f = p->pe.select(cand);
  if (out) {
    out->found = f.found;
    out->nof_ports = f.nof_ports;
    out->sfn_offset = f.sfn_offset;
    out->n_frames_used = f.n_frames_used;
    memcpy(out->bits, f.bits, sizeof(out->bits));
  }
  return f.found ? 1 : 0;
}

size_t mi_pbch_llr_floats(const mi_pbch_t* p) { return p ? p->pe.llr_floats() : 0; }

int mi_pbch_llr(mi_pbch_t* p, float* host, size_t n, int upload) {
  if (!p || !host || n > p->pe.llr_floats()) { mi::set_error("llr size"); return -1; }
  const bool ok = mi::hip_ok(hipStreamSynchronize(p->last), "sync") &&
                  (upload ? mi::hip_ok(hipMemcpy(p->pe.d_llr.p, host, n * 4, hipMemcpyHostToDevice), "H2D")
                          : mi::hip_ok(hipMemcpy(host, p->pe.d_llr.p, n * 4, hipMemcpyDeviceToHost), "D2H"));
  return ok ? 0 : -1;
}

}  // extern "C"
