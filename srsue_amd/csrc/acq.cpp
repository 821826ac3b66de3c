// acq.cpp -- cell acquisition (include/mi_dl.h): cell search, and the streaming search + MIB decode over a
// receive callback (mi_acq_*, below).  The cell search is what srsUE reaches through
// srslte_ue_cellsearch_scan (srsUE ue/src/phy/phch_recv.cc:137-220), batched over device-resident
// 1.92 Msps IQ on the sync front end's kernels (sync.hip): every lag of every 5 ms window is correlated with
// the three PSS roots in chunks of 64 lags, one launch; the SSS is detected at each (window, root) peak, one
// launch; the per-root statistics over the windows (srslte_ue_cellsearch_result_t) are host work.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "mi_dl.h"
#include "srslte/srslte.h"
#include "sync.h"

namespace {

constexpr uint32_t CS_PRB = 6, CS_N = 128, CS_HALF = 5 * 15 * CS_N;   // 9600 samples = 5 ms at 1.92 Msps
constexpr uint32_t CS_CHUNK = 64, CS_NCHUNK = CS_HALF / CS_CHUNK;     // 150 chunks of 64 lags

// the search over n_windows windows of iq (mi_cellsearch_run's contract) on engine e
int cellsearch(mi::SyncEngine& e, const float2* iq, const uint64_t* off, uint32_t n_windows, float threshold,
               mi_cell_result_t out[3], hipStream_t st) {
  if (!(threshold > 0.f)) threshold = MI_CELLSEARCH_THRESHOLD;
  const uint32_t sym5 = (uint32_t)mi::symbol_offset((int)CS_N, 5), sym6 = (uint32_t)mi::symbol_offset((int)CS_N, 6);
  // one job per (window, root, chunk): a chunk's maximum is what the peak-to-side ratio needs
  std::vector<mi::MiPssJob> jobs;
  jobs.reserve((size_t)n_windows * 3 * CS_NCHUNK);
  for (uint32_t w = 0; w < n_windows; w++)
    for (uint32_t u = 0; u < 3; u++)
      for (uint32_t c = 0; c < CS_NCHUNK; c++) jobs.push_back(mi::MiPssJob{off[w] + CS_CHUNK * c, CS_CHUNK, 1u << u});
  if (e.pss(iq, jobs, st)) return -1;
  struct Win { uint32_t lag; float rho, cfo, psr; bool sss; uint32_t nid1, sf5; };
  std::vector<Win> win((size_t)n_windows * 3);
  std::vector<mi::MiSssJob> sj;
  std::vector<uint32_t> sj_win;
  for (uint32_t w = 0; w < n_windows; w++)
    for (uint32_t u = 0; u < 3; u++) {
      const mi::MiPssRes* r = &e.pres[((size_t)w * 3 + u) * CS_NCHUNK];
      uint32_t bc = 0;
      for (uint32_t c = 1; c < CS_NCHUNK; c++)
        if (r[c].rho > r[bc].rho) bc = c;   // ties: the lower lag
      float side = 0.f;
      for (uint32_t c = 0; c < CS_NCHUNK; c++)
        if (c + 2 <= bc || c >= bc + 2) side = std::max(side, r[c].rho);
      Win& x = win[(size_t)w * 3 + u];
      x.lag = CS_CHUNK * bc + r[bc].lag;
      x.rho = r[bc].rho;
      x.cfo = r[bc].cfo;
      x.psr = side > 0.f ? r[bc].rho / side : 0.f;
      // the SSS symbol precedes the PSS symbol: it is detected only where it lies inside the window
      x.sss = x.lag + sym5 >= sym6;
      if (x.sss) {
        // start of the PSS's subframe; may lie before off[w] (the kernel reads symbols 5 and 6 only, which do not)
        sj.push_back(mi::MiSssJob{off[w] + x.lag - sym6, u, x.cfo});
        sj_win.push_back(w * 3 + u);
      }
    }
  if (e.sss(iq, sj, st)) return -1;
  for (size_t i = 0; i < sj.size(); i++) {
    win[sj_win[i]].nid1 = e.sres[i].nid1;
    win[sj_win[i]].sf5 = e.sres[i].sf5;
  }
  for (uint32_t u = 0; u < 3; u++) {
    mi_cell_result_t o;
    memset(&o, 0, sizeof(o));
    std::map<uint32_t, std::pair<uint32_t, double>> votes;   // cell id -> (windows, sum of peaks)
    for (uint32_t w = 0; w < n_windows; w++) {
      const Win& x = win[(size_t)w * 3 + u];
      if (!x.sss) continue;
      auto& v = votes[3 * x.nid1 + u];
      v.first++;
      v.second += x.rho;
    }
    uint32_t best_n = 0;
    double best_mean = -1.0;
    for (const auto& kv : votes) {
      const double mean = kv.second.second / kv.second.first;
      if (kv.second.first > best_n || (kv.second.first == best_n && mean > best_mean)) {
        best_n = kv.second.first;
        best_mean = mean;
        o.cell_id = kv.first;
      }
    }
    if (best_n) {
      double peak = 0, psr = 0, cfo = 0;
      int64_t sf0 = 0;
      for (uint32_t w = 0; w < n_windows; w++) {
        const Win& x = win[(size_t)w * 3 + u];
        if (!x.sss || 3 * x.nid1 + u != o.cell_id) continue;
        peak += x.rho;
        psr += x.psr;
        cfo += x.cfo;
        // the newest agreeing window wins: the last subframe-0 boundary at or before its PSS's subframe
        sf0 = (int64_t)(off[w] + x.lag) - (int64_t)sym6 - (x.sf5 ? (int64_t)CS_HALF : 0);
      }
      while (sf0 < 0) sf0 += 2 * (int64_t)CS_HALF;
      o.mode = (float)best_n / (float)n_windows;
      o.peak = (float)(peak / best_n);
      o.psr = (float)(psr / best_n);
      o.cfo = (float)(cfo / best_n);
      o.sf_start = (uint64_t)sf0;
      o.found = o.peak > threshold ? 1u : 0u;
    }
    out[u] = o;
  }
  return 0;
}

}  // namespace

struct mi_cellsearch {
  mi::SyncEngine eng;
};

// Streaming acquisition over a receive callback (what a radio user calls; one instance per thread, like
// srslte_ue_sync_t in ue_sync.cpp): a host ring of received samples, one non-blocking stream for every device
// operation of the instance, an internal batch of four 6-PRB 2-port subframe-0 slots for the PBCH frames.
struct mi_acq {
  mi::SyncEngine eng;
  hipStream_t st = nullptr;
  int (*recv)(void*, void*, uint32_t, srslte_timestamp_t*) = nullptr;
  void* handler = nullptr;
  std::vector<float2> ring;      // received samples [base, base + ring.size())
  uint64_t base = 0, pos = 0;    // pos: stream index of the next unread sample
  mi::DevBuf d_win, d_iq;
  mi_dl_batch_t* batch = nullptr;
  mi_pbch_t* pbch = nullptr;
  uint32_t batch_cell = 0xFFFFFFFFu;
};

namespace {

constexpr uint32_t SF_LEN = 15 * CS_N, FRAME = 2 * CS_HALF;

bool acq_fill(mi_acq* a, uint64_t upto) {
  const uint64_t have = a->base + a->ring.size();
  if (upto <= have) return true;
  const uint32_t n = (uint32_t)(upto - have);
  std::vector<float2> tmp(n);
  srslte_timestamp_t ts{};
  if (a->recv(a->handler, tmp.data(), n, &ts) < (int)n) { mi::set_error("acq: receive callback"); return false; }
  a->ring.insert(a->ring.end(), tmp.begin(), tmp.end());
  return true;
}

void acq_drop(mi_acq* a, uint64_t before) {
  if (before <= a->base) return;
  const uint64_t k = std::min<uint64_t>(before - a->base, a->ring.size());
  a->ring.erase(a->ring.begin(), a->ring.begin() + (ptrdiff_t)k);
  a->base += k;
}

// stream samples [from, from + n) -> d_win (the ring holds them)
bool acq_upload(mi_acq* a, uint64_t from, uint32_t n) {
  return a->d_win.ensure((size_t)n * sizeof(float2)) &&
         mi::hip_ok(hipMemcpyAsync(a->d_win.p, a->ring.data() + (from - a->base), (size_t)n * sizeof(float2),
                                   hipMemcpyHostToDevice, a->st),
                    "H2D");
}

// the internal PBCH batch of a cell: four subframe-0 slots, 6 PRB, 2 CRS ports estimated (a 1-port cell decodes
// under the 1-port hypothesis on port 0's estimates)
bool acq_batch(mi_acq* a, uint32_t cell_id) {
  if (a->batch && a->batch_cell == cell_id) return true;
  if (a->pbch) mi_pbch_destroy(a->pbch);
  if (a->batch) mi_dl_batch_destroy(a->batch);
  a->pbch = nullptr;
  a->batch = nullptr;
  mi_dl_sf_cfg_t c[4];
  memset(c, 0, sizeof(c));
  for (auto& x : c) {
    x.cell_id = cell_id; x.nof_prb = CS_PRB; x.nof_ports = 2; x.sf_idx = 0; x.cfi = 2; x.tm = 2; x.nl_td = 2;
    x.rnti = 1; x.tbs = 208; x.Qm = 2; x.new_tb = 1;
    for (uint32_t p = 0; p < CS_PRB; p++) x.prb_mask[p] = 1;
  }
  a->batch = mi_dl_batch_create(c, 4, 1, 0);
  if (!a->batch) return false;
  a->pbch = mi_pbch_create(a->batch);
  if (!a->pbch || !a->d_iq.ensure(mi_dl_batch_iq_samples(a->batch) * sizeof(float2))) return false;
  if (!mi::hip_ok(hipMemsetAsync(a->d_iq.p, 0, mi_dl_batch_iq_samples(a->batch) * sizeof(float2), a->st), "memset"))
    return false;
  a->batch_cell = cell_id;
  return true;
}

}  // namespace

extern "C" {

mi_cellsearch_t* mi_cellsearch_create(void) {
  auto* s = new mi_cellsearch();
  if (s->eng.init(CS_PRB)) { delete s; return nullptr; }
  return s;
}

void mi_cellsearch_destroy(mi_cellsearch_t* s) { delete s; }

int mi_cellsearch_run(mi_cellsearch_t* s, const void* d_iq, const uint64_t* off, uint32_t n_windows, float threshold,
                      mi_cell_result_t out[3], void* stream) {
  if (!s || !d_iq || !off || !out || n_windows == 0) { mi::set_error("mi_cellsearch_run: arguments"); return -1; }
  return cellsearch(s->eng, reinterpret_cast<const float2*>(d_iq), off, n_windows, threshold, out,
                    reinterpret_cast<hipStream_t>(stream));
}

mi_acq_t* mi_acq_create(int (*recv)(void*, void*, uint32_t, srslte_timestamp_t*), void* handler) {
  if (!recv) { mi::set_error("mi_acq_create: no receive callback"); return nullptr; }
  auto* a = new mi_acq();
  a->recv = recv;
  a->handler = handler;
  if (a->eng.init(CS_PRB) || !mi::hip_ok(hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking), "stream")) {
    mi_acq_destroy(a);
    return nullptr;
  }
  return a;
}

void mi_acq_destroy(mi_acq_t* a) {
  if (!a) return;
  if (a->st) (void)hipStreamSynchronize(a->st);
  if (a->pbch) mi_pbch_destroy(a->pbch);
  if (a->batch) mi_dl_batch_destroy(a->batch);
  if (a->st) (void)hipStreamDestroy(a->st);
  delete a;
}

int mi_acq_search(mi_acq_t* a, uint32_t n_half_frames, float threshold, mi_cell_result_t out[3], uint32_t* best) {
  if (!a || !out || n_half_frames == 0 || n_half_frames > 4096) { mi::set_error("mi_acq_search: arguments"); return -1; }
  const uint32_t len = n_half_frames * CS_HALF + CS_N;
  if (!acq_fill(a, a->pos + len) || !acq_upload(a, a->pos, len)) return -1;
  std::vector<uint64_t> off(n_half_frames);
  for (uint32_t w = 0; w < n_half_frames; w++) off[w] = (uint64_t)w * CS_HALF;
  if (cellsearch(a->eng, a->d_win.as<float2>(), off.data(), n_half_frames, threshold, out, a->st)) return -1;
  int nfound = 0;
  uint32_t b = 0;
  for (uint32_t u = 0; u < 3; u++) {
    out[u].sf_start += a->pos;   // stream index since the instance was created
    if (!out[u].found) continue;
    if (!nfound || out[u].peak > out[b].peak) b = u;
    nfound++;
  }
  if (best) *best = b;
  // the last symbol's worth of samples starts the next search window
  acq_drop(a, a->pos + (uint64_t)n_half_frames * CS_HALF);
  a->pos += (uint64_t)n_half_frames * CS_HALF;
  return nfound;
}

int mi_acq_mib(mi_acq_t* a, uint32_t cell_id, float cfo, uint32_t max_frames, mi_mib_t* mib) {
  if (!a || !mib || cell_id > 503 || max_frames == 0 || !(fabsf(cfo) < 1.0f)) {
    mi::set_error("mi_acq_mib: arguments");
    return -1;
  }
  const uint32_t nid2 = cell_id % 3, sym6 = (uint32_t)mi::symbol_offset((int)CS_N, 6);
  // the cell's subframe 0: PSS of N_ID_2 over a half frame in parallel chunks, SSS check (ue_sync.cpp's find)
  uint64_t sf0 = 0;
  bool have = false;
  for (int attempt = 0; attempt < 8 && !have; attempt++) {
    if (!acq_fill(a, a->pos + CS_HALF + CS_N) || !acq_upload(a, a->pos, CS_HALF + CS_N)) return -1;
    std::vector<mi::MiPssJob> jobs;
    constexpr uint32_t CH = 2048;
    for (uint32_t o = 0; o < CS_HALF; o += CH) jobs.push_back(mi::MiPssJob{o, std::min(CH, CS_HALF - o), 1u << nid2});
    if (a->eng.pss(a->d_win.as<float2>(), jobs, a->st)) return -1;
    uint32_t bi = 0;
    for (uint32_t i = 1; i < jobs.size(); i++)
      if (a->eng.pres[i].rho > a->eng.pres[bi].rho) bi = i;
    uint64_t s = a->pos + jobs[bi].off + a->eng.pres[bi].lag;   // stream index of the PSS useful part
    s = s >= sym6 + a->pos ? s - sym6 : s - sym6 + CS_HALF;      // boundary of the PSS's subframe
    if (!acq_fill(a, s + SF_LEN) || !acq_upload(a, s, SF_LEN)) return -1;
    if (a->eng.sss(a->d_win.as<float2>(), {mi::MiSssJob{0, nid2, cfo}}, a->st)) return -1;
    if (a->eng.sres[0].nid1 == cell_id / 3) {
      sf0 = a->eng.sres[0].sf5 ? s + CS_HALF : s;
      have = true;
    } else {   // another cell's PSS, or noise: the next half frame
      acq_drop(a, a->pos + CS_HALF);
      a->pos += CS_HALF;
    }
  }
  if (!have) return 0;
  if (!acq_batch(a, cell_id)) return -1;
  for (uint32_t i = 0; i < max_frames; i++) {
    const uint64_t s = sf0 + (uint64_t)i * FRAME;
    const uint32_t slot = i % 4;
    if (!acq_fill(a, s + SF_LEN)) return -1;
    acq_drop(a, s);
    a->pos = s;
    if (!acq_upload(a, s, SF_LEN) ||
        a->eng.correct(a->d_win.as<float2>(), a->d_iq.as<float2>(),
                       {mi::MiCfoJob{0, mi_dl_batch_iq_offset(a->batch, slot), cfo, 0}}, SF_LEN, a->st) ||
        mi_dl_batch_run_stages(a->batch, a->d_iq.p, a->st, (1u << MI_DL_STAGE_OFDM) | (1u << MI_DL_STAGE_CHEST)))
      return -1;
    // the growing candidate: the last min(i + 1, 4) frames' slots, oldest first
    const uint32_t n = std::min(i + 1, 4u);
    uint32_t sf[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < n; k++) sf[k] = (i - (n - 1) + k) % 4;
    mi_pbch_result_t r;
    if (mi_pbch_run(a->pbch, 1u, a->st) || mi_pbch_set_candidates(a->pbch, sf, &n, 1) || mi_pbch_run(a->pbch, 2u, a->st))
      return -1;
    const int rc = mi_pbch_result(a->pbch, 0, &r);
    if (rc < 0) return -1;
    a->pos = s + SF_LEN;
    if (rc == 0) continue;
    srslte_cell_t cell;
    memset(&cell, 0, sizeof(cell));
    uint32_t sfn = 0;
    srslte_pbch_mib_unpack(r.bits, &cell, &sfn);
    memset(mib, 0, sizeof(*mib));
    mib->nof_prb = cell.nof_prb;
    mib->nof_ports = r.nof_ports;
    mib->phich_length = (uint32_t)cell.phich_length;
    mib->phich_resources = (uint32_t)cell.phich_resources;
    mib->sfn = (sfn + r.sfn_offset) & 1023u;
    mib->n_frames = i + 1;
    mib->sf_start = s;
    memcpy(mib->bits, r.bits, sizeof(mib->bits));
    return 1;
  }
  return 0;
}

}  // extern "C"
