// emu.cpp -- TEST-ONLY host emulation of the per-lane kernel bodies (rm_body.h, tdec_body.h,
// tb_body.h) driven by the real planner.  Built into libsrsue_amd_emu.so with g++ -DMI_EMU; it is
// never linked into the product library.  Lanes of those kernels never communicate, so running
// each lane's code to completion in turn reproduces the GPU result operation for operation; the
// CPU test suite uses it to check planner + rate de-matching + turbo + TB assembly bit-exactly
// against the oracle without a GPU.  The per-work-item setup -- what turns (group or pair, lane) into a TdecArgs /
// TdecArgsP2, the output routing, the result write-back and the gather sources -- is not restated here: it is the
// MI_HD functions of tdec_body.h / tdec_p2_body.h that tdec.hip's kernels call, run on host arrays laid out as the
// device buffers are (one window-mask array of WM_STRIDE per group, dense pairs a fixed stride apart).
#include <algorithm>
#include <string.h>

#include <vector>

#include "csi_body.h"
#include "ctrl_rx_body.h"
#include "demap_body.h"
#include "kernels_consts.h"
#include "plan.h"
#include "rm_body.h"
#include "sm_body.h"
#include "tables.h"
#include "tb_body.h"
#include "tdec_body.h"
#include "tdec_p2_body.h"
#include "tdec_win_body.h"

static int g_q16 = 0;   // turbo arithmetic of the emulated decoder (MI_DL_FLAG_TDEC_I16)
extern "C" void emu_set_tdec_i16(int on) { g_q16 = on; }

static uint32_t crc8[256], crc8b[256];   // CRC24A / CRC24B byte tables

// crossed-schedule lane decoder (two wavefronts per group, tdec_body.h tdec_lane_x): 0 = off, 1 = register
// form, 2 = recompute form, 3 = two code blocks per lane (int16 only, tdec_p2_body.h)
static int g_x = 0;
extern "C" void emu_set_tdec_x(int on) { g_x = on; }
// packed decoder: waterfall compaction after iteration 0 (tdec_p2_body.h P2ContSrc; tdec.hip tdec_cont_*),
// continuation pairs filled in REVERSE lane order (the GPU's order depends on atomics: results may not)
static int g_compact = 0;
static uint64_t g_cont_cbs = 0;
extern "C" void emu_set_tdec_compact(int on) { g_compact = on; g_cont_cbs = 0; }
static int g_store_w = 0;   // compaction: the first launch stores its w rows, the continuation gathers them
extern "C" void emu_set_tdec_store_w(int on) { g_store_w = on; }
static int g_seg = 0;      // compaction rounds after the first: segmented, g_seg wavefronts per pair (tdec_kernel_p2s)
extern "C" void emu_set_tdec_seg(int s) { g_seg = s; }
static int g_rounds = 0;    // compaction: one iteration per round, the failing code blocks re-compacted between rounds
static uint64_t g_round_cbs = 0;
extern "C" void emu_set_tdec_rounds(int on) { g_rounds = on; g_round_cbs = 0; }
extern "C" uint64_t emu_round_codeblocks() { return g_round_cbs; }
extern "C" uint64_t emu_cont_codeblocks() { return g_cont_cbs; }
template <bool Q16>
static mi::TdecLaneResult emu_lane_x(const mi::TdecArgs& a, int lane) {
  mi::TdecExecHost ex;
  mi::TdecLaneResult r = g_x == 2 ? mi::tdec_lane_x<Q16, true>(a, lane, ex) : mi::tdec_lane_x<Q16, false>(a, lane, ex);
  r.tb_part = mi::tdec_pack(a, lane);
  return r;
}

// latency-form (segment-parallel) int16 decoder: threads per code block, 0 = off (tdec_win_body.h).
// Each phase of the GPU kernel (between two barriers) runs every segment in turn: within a phase a
// segment only reads what earlier phases wrote, so this reproduces the kernel exactly.
static uint32_t g_win = 0;
static uint64_t g_win_rounds = 0, g_win_halves = 0;
extern "C" void emu_set_tdec_win(uint32_t threads) { g_win = threads; g_win_rounds = g_win_halves = 0; }
extern "C" void emu_win_stats(uint64_t* rounds, uint64_t* halves) { *rounds = g_win_rounds; *halves = g_win_halves; }

template <bool DEC2>
static void emu_win_half(const mi::WinCb& c) {
  g_win_halves++;
  for (uint32_t j = 0; j < c.nseg; j++) mi::win_bwd_first<DEC2>(c, j);
  std::vector<float> v(8 * c.nseg);
  for (;;) {
    for (uint32_t j = 0; j + 1 < c.nseg; j++) mi::ck_get(c.bend + (j + 1) * 8, *reinterpret_cast<float(*)[8]>(&v[8 * j]));
    bool any = false;
    for (uint32_t j = 0; j + 1 < c.nseg; j++) any |= mi::win_bwd_fix<DEC2>(c, j, *reinterpret_cast<float(*)[8]>(&v[8 * j]));
    g_win_rounds++;
    if (!any) break;
  }
  for (uint32_t j = 0; j < c.nseg; j++) mi::win_fwd_first<DEC2>(c, j);
  for (;;) {
    for (uint32_t j = 1; j < c.nseg; j++) mi::ck_get(c.aend + (j - 1) * 8, *reinterpret_cast<float(*)[8]>(&v[8 * j]));
    bool any = false;
    for (uint32_t j = 1; j < c.nseg; j++) any |= mi::win_fwd_fix<DEC2>(c, j, *reinterpret_cast<float(*)[8]>(&v[8 * j]));
    g_win_rounds++;
    if (!any) break;
  }
}

// one code block (lane `lane` of group g) through the latency-form decoder, as tdec_win_kernel does
static mi::TdecLaneResult emu_win_cb(const MiGroupDesc& g, const MiKTab& kt, const MiLaneDesc& ld, const float* sbg,
                                     const uint32_t* kdata, uint32_t lane, uint32_t max_its, uint8_t* row) {
  const uint32_t K = g.K, P = g_win;
  mi::WinCb c;
  c.K = K;
  mi::win_geometry(K, P, c.S, c.nseg);
  std::vector<int16_t> q(3 * K + 12), d(K), w(K), bck((K / 4 + 1) * 8), ack((K / 4 + 1) * 8), bend(P * 8), aend(P * 8);
  std::vector<uint16_t> pi(K);
  std::vector<uint8_t> dec(K), pk(K / 8);
  c.q = q.data(); c.pi = pi.data(); c.d = d.data(); c.w = w.data(); c.dec = dec.data();
  c.bck = bck.data(); c.ack = ack.data(); c.bend = bend.data(); c.aend = aend.data();
  std::vector<uint8_t> lmap((g.Ncb + 15) / 16 * 16);
  c.lmap = lmap.data();
  for (uint32_t t = 0; t < P; t++) mi::win_load_map(c, t, P, sbg, g.Ncb);
  for (uint32_t t = 0; t < P; t++)
    mi::win_load(c, t, P, sbg, kdata + kt.pos_off, kdata + kt.pi_off, lane, ld.F);
  const uint32_t* tab = kdata + (ld.crc24a ? kt.crca_off : kt.crcb_off);
  mi::TdecLaneResult r{0, 0, 0};
  for (uint32_t it = 0; it < max_its; it++) {
    emu_win_half<false>(c);
    emu_win_half<true>(c);
    uint32_t x = 0;
    for (uint32_t t = 0; t < P; t++) x ^= mi::win_crc_part(c, t, P, tab);
    r.its = it + 1;
    r.crc_ok = x == 0;
    if (r.crc_ok) break;
  }
  for (uint32_t t = 0; t < P; t++) mi::win_pack(c, t, P, pk.data());
  memcpy(row, pk.data(), K / 8);
  const uint32_t b0 = ld.F / 8, b1 = K / 8 - (ld.crc24a ? 0 : 3);
  for (uint32_t t = 0; t < P; t++) r.tb_part ^= mi::win_tb_term(c, t, P, pk.data(), b0, b1, crc8);
  return r;
}

// softbuffer arena kept from one emu_decode_llr call to the next (retransmissions: new_tb = 0 lanes combine with it)
static int g_keep_sb = 0;
static std::vector<float> g_sb;
extern "C" void emu_keep_softbuffer(int on) { g_keep_sb = on; g_sb.clear(); }
// the kept arena (the layout of MI_DL_BUF_SOFTBUFFER): its size in floats; copied to out when out is not null
extern "C" size_t emu_softbuffer(float* out) {
  if (out && !g_sb.empty()) memcpy(out, g_sb.data(), g_sb.size() * sizeof(float));
  return g_sb.size();
}

extern "C" int emu_decode_llr(const mi_dl_sf_cfg_t* cfgs, uint32_t n, const float* llr_concat, uint32_t max_its,
                              uint8_t* payload, uint32_t* tb_ok, uint32_t* tb_its, uint32_t* cb_its) {
  mi::crc24_fill_tables(crc8, crc8b, 0, 1);
  mi::Plan P;
  if (P.build(cfgs, n, true)) return -1;
  std::vector<float> e(P.e_floats, 0.f), sb_call, scr(P.scratch_floats, 0.f);
  // HARQ: the kept softbuffer arena lives across calls while the layout's size stays (a batch's arena across runs)
  std::vector<float>& sb = g_keep_sb ? g_sb : sb_call;
  if (sb.size() != P.sb_floats) sb.assign(P.sb_floats, 0.f);
  std::vector<uint8_t> dec(P.dec_bytes, 0), cbb(P.lanes.size() * mi::CB_BYTES_STRIDE, 0);
  std::vector<uint32_t> cits(P.lanes.size(), 0), ccrc(P.lanes.size(), 0), ctbp(P.lanes.size(), 0);
  size_t src = 0;
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t G = P.pds[P.sfs[s].pdsch].G;
    memcpy(&e[P.sfs[s].e_off], llr_concat + src, G * sizeof(float));
    src += G;
  }
  // rate de-matching and the window masks of every group (rm.hip, tdec.hip rowmask_kernel), then the decoders on the
  // buffers and tables laid out as the kernels get them
  std::vector<uint32_t> wm(P.groups.size() * mi::WM_STRIDE, 0u);
  for (size_t gi = 0; gi < P.groups.size(); gi++) {
    const MiGroupDesc& g = P.groups[gi];
    float* sbg = &sb[g.sb_off];
    const uint8_t* map = reinterpret_cast<const uint8_t*>(sbg + mi::sb_map_off(g.Ncb));
    const MiKTab& kt = P.ktabs[g.ktab];
    for (uint32_t p = 0; p < g.Ncb; p++)
      mi::rm_combine_row(&P.lanes[g.lane0], P.kdata.data(), e.data(), sbg, g.Ncb, p, &P.kdata[kt.ipos_off]);
    for (uint32_t w = 0; w <= g.K / mi::BETA_W; w++)
      wm[gi * mi::WM_STRIDE + w] = mi::tdec_window_mask(map, &P.kdata[kt.pos_off], w);
  }
  const bool p2 = g_x == 3 && g_q16;   // two code blocks per lane (tdec_p2_body.h): its runs go to the payload in place
  const mi::TdecMem m{sb.data(), wm.data(), scr.data(), dec.data(), cbb.data(), p2 ? payload : nullptr, P.kdata.data()};
  if (p2) {
    std::vector<uint32_t> stash((size_t)mi::P2_STASH_ROWS * mi::LANES);
    const uint32_t its1 = g_compact && max_its > 1 ? 1 : max_its;   // tdec.hip launch_tdec_p2, as Engine::launch_turbo
    for (size_t pp = 0; pp < P.pairs.size(); pp += 2) {
      const uint32_t ga = P.pairs[pp], gbi = P.pairs[pp + 1];
      const MiGroupDesc &gA = P.groups[ga], &gB = P.groups[gbi != 0xFFFFFFFFu ? gbi : ga];
      for (int lane = 0; lane < mi::LANES; lane++) {
        const uint32_t li[2] = {gA.lane0 + lane, gB.lane0 + lane};
        const MiLaneDesc &l0 = P.lanes[li[0]], &l1 = P.lanes[li[1]];
        mi::TdecArgsP2 a;
        a.live = mi::p2_first_live(gbi, l0, l1);
        if (!a.live) continue;
        mi::p2_first_args(a, m, ga, gbi, gA, gB, P.ktabs[gA.ktab], li, l0, l1, crc8, crc8b, its1, 1,
                          its1 == 1 && !g_store_w);
        a.stash = stash.data();   // the LDS stash of the 16-step spans (one lane at a time here)
        mi::TdecP2ExecHost ex;
        // the spacing of tdec.hip tdec_kernel_p2x: 16-step spans
        const mi::TdecP2Result r = its1 == 1 ? mi::tdec_p2_lane<false, mi::P2_CKS, true>(a, lane, ex)
                                             : mi::tdec_p2_lane<false, mi::P2_CKS>(a, lane, ex);
        mi::p2_put_result(a.live, li, r, cits.data(), ccrc.data(), ctbp.data());
      }
    }
    if (g_compact && max_its > 1) {
      // each group's pair (its first group) and half
      std::vector<uint32_t> pa(P.groups.size()), ph(P.groups.size());
      for (size_t pp = 0; pp < P.pairs.size(); pp += 2)
        for (int h = 0; h < 2; h++)
          if (P.pairs[pp + h] != 0xFFFFFFFFu) { pa[P.pairs[pp + h]] = P.pairs[pp]; ph[P.pairs[pp + h]] = h; }
      std::vector<uint32_t> ks;
      for (const MiGroupDesc& g : P.groups)
        if (std::find(ks.begin(), ks.end(), g.K) == ks.end()) ks.push_back(g.K);
      for (uint32_t K : ks) {
        std::vector<uint32_t> cont;   // continuing code blocks of this K, reverse lane order
        for (size_t gi = P.groups.size(); gi-- > 0;)
          if (P.groups[gi].K == K)
            for (int l = mi::LANES - 1; l >= 0; l--) {
              const uint32_t li = P.groups[gi].lane0 + l;
              if (P.lanes[li].valid && !ccrc[li]) cont.push_back(li);
            }
        g_cont_cbs += cont.size();
        const uint32_t gi0 = [&] { uint32_t g = 0; while (P.groups[g].K != K) g++; return g; }();
        const MiKTab& kt = P.ktabs[P.groups[gi0].ktab];
        const uint32_t* pos = &P.kdata[kt.pos_off];
        const size_t PU = (size_t)(7 * K + 20) * mi::LANES;   // tdec.hip: a dense continuation pair
        auto npairs = [](size_t cbs) { return (cbs + 2 * mi::LANES - 1) / (2 * mi::LANES); };
        // the live halves of lane `lane` of dense pair p of a list of cbs code blocks, and each one's slot
        auto slots = [](size_t cbs, size_t p, int lane, size_t (&d)[2]) {
          uint32_t live = 0;
          for (int h = 0; h < 2; h++) {
            d[h] = p * 2 * mi::LANES + (size_t)h * mi::LANES + lane;
            if (d[h] < cbs) live |= 1u << h;
          }
          return live;
        };
        std::vector<uint32_t> bufs(npairs(cont.size()) * PU, 0u);   // dense pair p at p PU
        // round 1's gather (tdec_cont_gather_kernel): q rows from the softbuffer, w or x2 rows from the source pairs
        for (size_t p = 0; p < npairs(cont.size()); p++)
          for (int lane = 0; lane < mi::LANES; lane++) {
            size_t d[2];
            const uint32_t live = slots(cont.size(), p, lane, d);
            if (!live) continue;
            mi::P2ContSrc src[2] = {};
            for (int h = 0; h < 2; h++)
              if ((live >> h) & 1u) {
                const uint32_t g = cont[d[h]] / mi::LANES;
                src[h] = mi::p2_cont_src(m.sb, m.wm, m.scratch, P.groups.data(), cont[d[h]], pa[g], ph[g]);
              }
            uint32_t* cscr = &bufs[p * PU];
            uint32_t* cq = &cscr[(size_t)(4 * K + 8) * mi::LANES];
            for (uint32_t w = 0; w < mi::p2_cont_qwins(K); w++) {
              uint32_t q[3 * mi::BETA_W];
              mi::p2_cont_qwin(src, live, pos, w, q);
              for (int i = 0; i < 3 * mi::BETA_W; i++) cq[(size_t)(3 * mi::BETA_W * w + i) * mi::LANES + lane] = q[i];
            }
            for (uint32_t k = 0; k < K; k++) {
              if (g_store_w) cscr[(size_t)k * mi::LANES + lane] = mi::p2_cont_wrow(src, live, k);
              else cscr[(size_t)(K + k) * mi::LANES + lane] = mi::p2_cont_xrow(src, live, K, k);
            }
          }
        // iterations it0 .. it_end - 1 of every dense pair (tdec_kernel_p2c, or segmented: tdec_kernel_p2s)
        std::vector<uint32_t> segv((size_t)4 * 64 * mi::P2_CKW * mi::LANES);   // the segmented form's boundary vectors
        auto run_pairs = [&](std::vector<uint32_t>& pb, const std::vector<uint32_t>& list, uint32_t it0,
                             uint32_t it_end) {
          const size_t dstride = (size_t)K * mi::LANES;
          std::vector<uint8_t> cdec(npairs(list.size()) * dstride, 0);
          std::vector<uint32_t> dl(1, (uint32_t)list.size());   // the device's list: its count, then the lane indices
          dl.insert(dl.end(), list.begin(), list.end());
          for (size_t p = 0; p < npairs(list.size()); p++)
            for (int lane = 0; lane < mi::LANES; lane++) {
              mi::TdecArgsP2 a{};
              uint32_t li[2];
              // (the segmented kernel's form of the mapping also serves lanes without code blocks: none decoded here)
              a.live = g_seg && it0 > 1 ? mi::p2_cont_lanes<true>(li, dl.data(), dl[0], (uint32_t)p, lane)
                                        : mi::p2_cont_lanes<false>(li, dl.data(), dl[0], (uint32_t)p, lane);
              if (!a.live) continue;
              mi::p2_cont_args(a, li, (uint32_t)p, pb.data(), PU, cdec.data(), dstride, m.cb_bytes, m.payload,
                               P.lanes.data(), m.kdata, kt, crc8, crc8b, K, max_its, it0 > 1 || g_store_w, it0, it_end);
              mi::TdecP2ExecHost ex;
              mi::TdecP2Result r;
              if (g_seg && it0 > 1) {
                // tdec.hip tdec_kernel_p2s: the segments of one lane in turn, fix-up rounds until nothing changes
                const size_t vw = (size_t)g_seg * mi::P2_CKW * mi::LANES;
                mi::P2SegVecs V{&segv[0], &segv[vw], &segv[2 * vw], &segv[3 * vw]};
                mi::p2s_half_host<false>(a, lane, (uint32_t)g_seg, V);
                mi::p2s_half_host<true>(a, lane, (uint32_t)g_seg, V);
                r = mi::p2s_check(a, lane);
              } else {
                // tdec.hip launch_tdec_cont: 4-step checkpoints in the rounds after the first
                r = it0 > 1 ? mi::tdec_p2_lane<true, mi::P2C_CKS_LATE>(a, lane, ex)
                            : mi::tdec_p2_lane<true, mi::P2C_CKS>(a, lane, ex);
              }
              mi::p2_put_result(a.live, li, r, cits.data(), ccrc.data(), ctbp.data());
            }
        };
        if (!g_rounds) {
          run_pairs(bufs, cont, 1, max_its);
          continue;
        }
        // re-compaction rounds (tdec.hip launch_tdec_cont): one iteration each, the code blocks still failing
        // gathered -- here in reverse slot order, so again with new partners -- into fewer dense pairs
        run_pairs(bufs, cont, 1, 2);
        for (uint32_t it = 2; it < max_its; it++) {
          std::vector<uint32_t> next, srcs;
          for (size_t d = cont.size(); d-- > 0;)
            if (!ccrc[cont[d]]) { next.push_back(cont[d]); srcs.push_back((uint32_t)d); }
          g_round_cbs += next.size();
          std::vector<uint32_t> nb(npairs(next.size()) * PU, 0u);
          for (size_t p = 0; p < npairs(next.size()); p++)   // tdec_cont_gather2_kernel
            for (int lane = 0; lane < mi::LANES; lane++) {
              size_t d[2];
              const uint32_t live = slots(next.size(), p, lane, d);
              if (!live) continue;
              mi::P2ContSrc src[2] = {};
              for (int h = 0; h < 2; h++)
                if ((live >> h) & 1u) src[h] = mi::p2_cont_src2(bufs.data(), PU, srcs[d[h]]);
              uint32_t* dp = &nb[p * PU];
              for (uint32_t r = 0; r < K; r++) dp[(size_t)r * mi::LANES + lane] = mi::p2_cont_drow(src, live, r);
              for (uint32_t r = 0; r < 3 * (K + 4); r++) {
                const size_t row = (size_t)(4 * K + 8) + r;
                dp[row * mi::LANES + lane] = mi::p2_cont_drow(src, live, row);
              }
            }
          run_pairs(nb, next, it, it + 1);
          cont.swap(next);
          bufs.swap(nb);
        }
      }
    }
  }
  for (size_t gi = 0; gi < P.groups.size() && !p2; gi++) {
    const MiGroupDesc& g = P.groups[gi];
    const MiKTab& kt = P.ktabs[g.ktab];
    for (int lane = 0; lane < mi::LANES; lane++) {
      const uint32_t li = g.lane0 + lane;
      const MiLaneDesc& ld = P.lanes[li];
      if (!ld.valid) continue;
      mi::TdecArgs a;
      mi::tdec_lane_args(a, m, (uint32_t)gi, g, kt, li, ld, crc8, max_its, 1);
      mi::TdecLaneResult r = g_win && g_q16 ? emu_win_cb(g, kt, ld, a.sb, m.kdata, lane, max_its, a.cb_bytes)
                           : g_x ? (g_q16 ? emu_lane_x<true>(a, lane) : emu_lane_x<false>(a, lane))
                           : g_q16 ? mi::tdec_lane<true>(a, lane) : mi::tdec_lane<false>(a, lane);
      cits[li] = r.its;
      ccrc[li] = r.crc_ok;
      ctbp[li] = r.tb_part;
    }
  }
  for (uint32_t t = 0; t < n; t++) {
    const MiTbDesc& tb = P.tbs[t];
    const uint32_t* lanes = &P.cb_list[tb.cb_list];
    std::vector<uint8_t> buf;
    for (uint32_t r = 0; r < tb.C; r++) {
      const uint8_t* src = &cbb[(size_t)lanes[r] * mi::CB_BYTES_STRIDE + (r == 0 ? tb.F / 8 : 0)];
      buf.insert(buf.end(), src, src + mi::tb_cb_nbytes(tb, r));
    }
    if (!p2) memcpy(payload + tb.pay_off, buf.data(), tb.tbs / 8);   // p2: written in place
    // TB CRC from the decoder's per-code-block partial registers (tb_kernel's formulation)
    uint32_t crc = 0;
    for (uint32_t r = 0; r < tb.C; r++) crc ^= mi::tb_crc_term(tb, r, ctbp[lanes[r]]);
    tb_ok[t] = crc == 0;
    uint32_t its = 0;
    for (uint32_t r = 0; r < tb.C; r++) its = cits[lanes[r]] > its ? cits[lanes[r]] : its;
    tb_its[t] = its;
  }
  if (cb_its) memcpy(cb_its, cits.data(), cits.size() * 4);
  return 0;
}

extern "C" size_t emu_payload_offset(const mi_dl_sf_cfg_t* cfgs, uint32_t n, uint32_t sf) {
  mi::Plan P;
  if (P.build(cfgs, n, true)) return 0;
  return P.tbs[sf].pay_off;
}

// The G LLRs of one PDSCH subframe from n_rx antennas' grids ([n_rx][14][W] float2) and channel estimates
// ([n_rx][ports][14][W] float2): demap_body.h demap_llr -- the kernels' equalisation with antenna combining, demapper
// and descrambling -- over the planner's RE list and scrambling words, bit by bit.  out: G floats.  Returns G, -1 on a
// bad configuration or antenna count.
template <int NRX>
static void emu_llr_run(const MiPdschDesc& pd, const float2* g, const float2* c0, size_t W, const uint32_t* re,
                        const uint32_t* scr, float noise, size_t g_rx, size_t c_rx, float* out) {
  const float2* c1 = c0 + (size_t)mi::NSYMB * W;
  for (uint32_t gi = 0; gi < pd.G; gi++)
    out[gi] = pd.Qm == 2   ? mi::demap_llr<2, NRX>(pd, gi, g, c0, c1, re, scr, noise, g_rx, c_rx)
              : pd.Qm == 4 ? mi::demap_llr<4, NRX>(pd, gi, g, c0, c1, re, scr, noise, g_rx, c_rx)
                           : mi::demap_llr<6, NRX>(pd, gi, g, c0, c1, re, scr, noise, g_rx, c_rx);
}
extern "C" int emu_pdsch_llr_rx(const mi_dl_sf_cfg_t* cfg, uint32_t n_rx, const float* grids, const float* ces,
                                float noise, float* out) {
  mi::Plan P;
  if (n_rx < 1 || n_rx > 2 || P.build(cfg, 1, true)) return -1;
  const MiPdschDesc& pd = P.pds[P.sfs[0].pdsch];
  const size_t W = 12 * (size_t)cfg->nof_prb, g_rx = (size_t)mi::NSYMB * W, c_rx = g_rx * cfg->nof_ports;
  const float2* g = reinterpret_cast<const float2*>(grids);
  const float2* c0 = reinterpret_cast<const float2*>(ces);
  const uint32_t *re = &P.re_tab[pd.re_off], *scr = &P.scr_tab[pd.scr_off];
  if (n_rx == 2) emu_llr_run<2>(pd, g, c0, W, re, scr, noise, g_rx, c_rx, out);
  else emu_llr_run<1>(pd, g, c0, W, re, scr, noise, g_rx, c_rx, out);
  return (int)pd.G;
}

// What the planner lays out for entry sf of a batch (tests/test_sm_plan.py): out[0..3] = its IQ, grid, ce and LLR
// offsets, [4] G, [5] RE count, [6] code blocks, [7] / [8] / [9] the sum, smallest and largest E of its code blocks,
// [10] payload offset, [11] 1 when an FFT list holds it, then the batch's totals: [12] IQ samples, [13] grid and
// [14] ce elements, [15] LLR floats, [16] FFT list entries, [17] channel-estimation list entries (0 = every entry),
// [18] codeword pairs, [19] the largest demap unit count.  Returns 0, -1 when the planner refuses (emu_last_error).
extern "C" int emu_plan_info(const mi_dl_sf_cfg_t* cfgs, uint32_t n, uint32_t sf, uint64_t* out) {
  mi::Plan P;
  if (P.build(cfgs, n, true) || sf >= n) return -1;
  const MiSfDesc& sd = P.sfs[sf];
  const MiPdschDesc& pd = P.pds[sd.pdsch];
  uint64_t sum = 0, lo = ~0ull, hi = 0;
  for (const MiLaneDesc& ld : P.lanes)
    if (ld.valid && ld.tb == sf) {
      sum += ld.E;
      lo = std::min<uint64_t>(lo, ld.E);
      hi = std::max<uint64_t>(hi, ld.E);
    }
  const bool in_fft = std::find(P.fft_list_flat.begin(), P.fft_list_flat.end(), sf) != P.fft_list_flat.end();
  const uint64_t v[20] = {sd.iq_off, sd.grid_off, sd.ce_off, sd.e_off, pd.G, pd.nre, P.tbs[sf].C, sum, lo, hi,
                          P.tbs[sf].pay_off, in_fft, P.iq_samples, P.grid_elems, P.ce_elems, P.e_floats,
                          P.fft_list_flat.size(), P.phys.size(), P.sm.size(), P.max_units};
  memcpy(out, v, sizeof(v));
  return 0;
}
extern "C" const char* emu_last_error() { return mi::last_error(); }

// The LLRs of both codewords of one spatially multiplexed subframe (cfg_pair: its cw 0 and cw 1 entries) from the two
// antennas' grids ([2][14][W] float2) and channel estimates ([2][2][14][W] float2): sm_body.h sm_detect_re -- the
// arithmetic of sm_detect_kernel -- RE by RE over the planner's pair descriptor.  out0 / out1: nre Qm0 and nre Qm1
// floats.  Returns nre, -1 on a configuration the planner refuses.
extern "C" int emu_pdsch_llr_sm(const mi_dl_sf_cfg_t* cfg_pair, const float* grids, const float* ces, float noise,
                                float* out0, float* out1) {
  mi::Plan P;
  if (P.build(cfg_pair, 2, true) || P.sm.size() != 1) return -1;
  const MiSmDesc& d = P.sm[0];
  const size_t W = 12 * (size_t)cfg_pair->nof_prb, g_rx = (size_t)mi::NSYMB * W, c_rx = 2 * g_rx;
  std::vector<float> e(P.e_floats, 0.f);
  for (uint32_t i = 0; i < d.nre; i++)
    mi::sm_detect_re(d, i, reinterpret_cast<const float2*>(grids) + d.goff, reinterpret_cast<const float2*>(ces) + d.coff,
                     P.re_tab.data(), P.scr_tab.data(), e.data(), noise, g_rx, c_rx);
  memcpy(out0, &e[d.e0], (size_t)d.nre * d.qm0 * sizeof(float));
  memcpy(out1, &e[d.e1], (size_t)d.nre * d.qm1 * sizeof(float));
  return (int)d.nre;
}

// The 8 M PDCCH soft bits of one subframe, in logical (CCE) order, from n_rx antennas' grids ([n_rx][14][W] float2) and
// channel estimates ([n_rx][ports][14][W] float2): ctrl_rx_body.h pdcch_reg_llr_rx -- the arithmetic of the two-antenna
// pdcch_llr_kernel, REG by REG -- over the planner's REG list, quadruplet permutation and scrambling words (tables.cpp,
// as CtrlEngine::build lays them out).  out: 8 M floats.  Returns M, -1 on a bad cell, CFI or antenna count.
template <int NRX>
static void emu_pdcch_run(uint32_t M, uint32_t ports, size_t W, const float2* g, const float2* c0, const uint32_t* re,
                          const uint32_t* lg, const uint32_t* scr, float noise, float* out) {
  const size_t g_rx = (size_t)mi::NSYMB * W, c_rx = g_rx * ports;
  for (uint32_t i = 0; i < M; i++) {
    const uint32_t q = lg[i], sw = scr[q / 4] >> (8 * (q % 4));
    mi::pdcch_reg_llr_rx<NRX>(g, c0, c0 + g_rx, re + 4 * i, ports == 2, noise, g_rx, c_rx, sw, out + 8 * (size_t)q);
  }
}
extern "C" int emu_pdcch_llr_rx(uint32_t cell_id, uint32_t nof_prb, uint32_t nof_ports, uint32_t phich_ng, uint32_t cfi,
                                uint32_t sf_idx, uint32_t n_rx, const float* grids, const float* ces, float noise,
                                float* out) {
  if (n_rx < 1 || n_rx > 2 || nof_ports < 1 || nof_ports > 2 || cfi < 1 || cfi > 3 || phich_ng > 3 || sf_idx > 9 ||
      cell_id > 503 || !mi::std_nof_prb(nof_prb))
    return -1;
  std::vector<uint32_t> re4, lg;
  const uint32_t M = mi::pdcch_regs(cell_id, nof_prb, phich_ng, cfi, &re4);
  mi::pdcch_quad_perm(M, cell_id, lg);
  std::vector<uint32_t> scr((8 * M + 31) / 32);
  mi::gold_words(sf_idx * 512 + cell_id, 8 * M, scr.data());
  const float2* g = reinterpret_cast<const float2*>(grids);
  const float2* c0 = reinterpret_cast<const float2*>(ces);
  if (n_rx == 2) emu_pdcch_run<2>(M, nof_ports, 12 * (size_t)nof_prb, g, c0, re4.data(), lg.data(), scr.data(), noise, out);
  else emu_pdcch_run<1>(M, nof_ports, 12 * (size_t)nof_prb, g, c0, re4.data(), lg.data(), scr.data(), noise, out);
  return (int)M;
}

// The CSI record of one subframe (csi_body.h: the arithmetic of csi_kernel, point by point) from its channel estimates
// ces ([n_rx][ports][rows][W] float2, rows = 14, or 4 when compact: the pilot rows only) and noise n.  Returns 0, -1 on a
// bad port / antenna count or bandwidth.
extern "C" int emu_csi(uint32_t nof_prb, uint32_t ports, uint32_t n_rx, int compact, const float* ces, float noise,
                       mi_dl_csi_result_t* out) {
  MiCsiSf d{};
  if (ports < 1 || ports > 2 || n_rx < 1 || n_rx > 2 || !mi::csi_subbands(nof_prb, &d.sb_prb, &d.n_sb)) return -1;
  d.W = 12 * nof_prb;
  d.ports = ports;
  const uint32_t mask = mi::csi_valid_mask(ports, n_rx), rows = compact ? 4 : mi::NSYMB;
  const size_t port = (size_t)rows * d.W, c_rx = port * ports;
  const float2* c = reinterpret_cast<const float2*>(ces);
  const float2 zero = make_float2(0.f, 0.f);
  noise = fmaxf(noise, 1e-9f);
  const float inv_n = 1.0f / noise;
  float sums[1 + MI_CSI_MAX_SB][mi::CSI_NACC] = {};
  const uint32_t n_chunk = d.n_sb ? d.n_sb : 1u, cw = d.n_sb ? 12u * d.sb_prb : d.W;
  for (uint32_t ch = 0; ch < n_chunk; ch++) {
    const uint32_t k0 = ch * cw, k1 = ch + 1 == n_chunk ? d.W : k0 + cw;
    for (int r = 0; r < 4; r++) {
      float acc[mi::CSI_NACC] = {};
      const float2* c00 = c + (size_t)(compact ? r : mi::CE_PL[r]) * d.W;
      for (uint32_t k = k0; k < k1; k++)
        mi::csi_point(c00[k], ports == 2 ? c00[port + k] : zero, n_rx == 2 ? c00[c_rx + k] : zero,
                      ports == 2 && n_rx == 2 ? c00[c_rx + port + k] : zero, mask, inv_n, acc);
      for (int i = 0; i < mi::CSI_NACC; i++) sums[1 + ch][i] += acc[i];
    }
    for (int i = 0; i < mi::CSI_NACC; i++) sums[0][i] += sums[1 + ch][i];
  }
  memset(out, 0, sizeof(*out));
  for (uint32_t t = 0; t < (uint32_t)mi::CSI_CELLS; t++) mi::csi_cell(t, sums, d, mask, out);
  mi::csi_decide(sums[0], d, mask, noise, out);
  return 0;
}

// The packed decoder's trellis start (tdec_p2_body.h header, p2.h tadd_a): the LLRs of steps 0..2 taken from the start
// state with the saturating alpha adds and no masking of the unreachable states, against the float recursion with -inf
// (the oracle's semantics, oracle/o_fec.c), at adversarial magnitudes -- inputs drawn at the quantiser's clamps half of
// the time and beta vectors from backward recursions over such inputs (the running beta of phase 2: 0..3 unnormalised
// steps after a window normalisation).  ninf: the start value of the unreachable alpha states (the product's is
// Metric<P2>::ninf_alpha(), -32768; a weaker one must fail, which shows the draws reach the margin).  Returns the number
// of (trial, step, half) LLRs -- of llr_step and of alpha_step -- that differ.
extern "C" uint64_t emu_p2_start_llr_check(uint64_t seed, uint32_t trials, int ninf) {
  uint64_t st = seed | 1u, bad = 0;
  auto rnd = [&]() {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(st >> 33);
  };
  auto pick = [&](int lim) {
    const uint32_t r = rnd();
    if (r & 1u) return (r & 2u) ? lim : -lim;
    return (int)(rnd() % (uint32_t)(2 * lim + 1)) - lim;
  };
  const int XS = 1535, XP = (int)mi::I16_CI;   // DEC2's systematic clamp (DEC1: 511 + 1023), the parity quantiser
  for (uint32_t t = 0; t < trials; t++) {
    float bf[2][8], xsf[2][3], xpf[2][3];
    for (int h = 0; h < 2; h++) {
      for (int s = 0; s < 8; s++) bf[h][s] = 0.f;
      const int n = 4 + 4 * (int)(rnd() % 4), extra = (int)(rnd() % 4);
      for (int i = 0; i < n + extra; i++) {
        float nb[8];
        mi::beta_step<false>(bf[h], (float)pick(XS), (float)pick(XP), nb);
        for (int s = 0; s < 8; s++) bf[h][s] = nb[s];
        if (i < n && (i & 3) == 3) mi::norm8<true>(bf[h]);
      }
      for (int k = 0; k < 3; k++) {
        xsf[h][k] = (float)pick(XS);
        xpf[h][k] = (float)pick(XP);
      }
    }
    mi::P2 bp[8], ap[8];
    float af[2][8];
    for (int s = 0; s < 8; s++) {
      bp[s] = mi::p2_make((int)bf[0][s], (int)bf[1][s]);
      ap[s] = s ? mi::p2_make(ninf, ninf) : mi::Metric<mi::P2>::zero();
      for (int h = 0; h < 2; h++) af[h][s] = s ? -INFINITY : 0.f;
    }
    for (int k = 0; k < 3; k++) {
      const mi::P2 xs = mi::p2_make((int)xsf[0][k], (int)xsf[1][k]), xp = mi::p2_make((int)xpf[0][k], (int)xpf[1][k]);
      const mi::P2 lp = mi::llr_step(ap, bp, xs, xp);
      mi::P2 ap2[8];
      for (int s = 0; s < 8; s++) ap2[s] = ap[s];
      const mi::P2 lp2 = mi::alpha_step<false>(ap2, bp, xs, xp);
      for (int h = 0; h < 2; h++) {
        float a2[8];
        for (int s = 0; s < 8; s++) a2[s] = af[h][s];
        const float lf = mi::alpha_step<false>(a2, bf[h], xsf[h][k], xpf[h][k]);
        const int lo = h ? mi::p2_hi(lp) : mi::p2_lo(lp), lo2 = h ? mi::p2_hi(lp2) : mi::p2_lo(lp2);
        bad += (float)lo != lf;
        bad += (float)lo2 != lf;
      }
      // both recursions one step on (the next step's alpha), the reachable states checked on the way
      mi::alpha_fwd<false>(ap, xs, xp);
      for (int h = 0; h < 2; h++) {
        mi::alpha_fwd<false>(af[h], xsf[h][k], xpf[h][k]);
        for (int s = 0; s < 8; s++)
          if (af[h][s] != -INFINITY) bad += (float)(h ? mi::p2_hi(ap[s]) : mi::p2_lo(ap[s])) != af[h][s];
      }
      // and the beta of the next (lower) step from this one's inputs, as phase 2 walks backwards -- kept as drawn: any
      // vector of bounded spread stands for beta_{k+1}
    }
  }
  return bad;
}
