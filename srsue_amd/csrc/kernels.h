// kernels.h -- host launchers of the gfx950 kernels of the DL PDSCH path.
// The turbo launchers take the stage's buffers as typed views (TdecBufs, TdecContBufs, TdecContSched) and unpack them
// into their kernels' individual __restrict__ pointer parameters.
#pragma once
#include <hip/hip_runtime.h>
#include "dl_common.h"
#include "kernels_consts.h"

namespace mi {

// Receive antennas of a batch (receive diversity): the IQ, grid, channel-estimate and metrics buffers hold n
// consecutive planes, each laid out as the single-antenna buffer; antenna a of a subframe lives at the subframe's
// offset + a x the plane stride (IQ samples, float2 grid / estimate elements; metrics: 5 floats per (antenna,
// subframe)).  Uniform over a launch: kernel arguments, no descriptor carries them.
struct RxPlanes {
  uint32_t n = 1;
  size_t iq = 0, grid = 0, ce = 0;
};
// OFDM RX (srslte_ofdm_rx_sf): one workgroup per (subframe, antenna), 14 FFTs of size N
void launch_ofdm_rx(int N, const void* iq, bool sc16, float2* grid, const MiSfDesc* sfs, const uint32_t* list,
                    uint32_t n, const float2* tw, uint32_t W, const RxPlanes& rx, hipStream_t st);
// channel estimation (srslte_chest_dl_estimate): one workgroup per (subframe, antenna), all ports
// list (n_list entries; nullptr = all n_sf): the subframes to estimate -- a batch with codeword pairs leaves out the
// cw = 1 entries, whose estimates are their partners'; the metrics rows stay indexed by subframe
void launch_chest(const float2* grid, float2* ce, const MiSfDesc* sfs, const MiCellDesc* cells,
                  const float2* crs, float* metrics, uint32_t n_sf, const RxPlanes& rx, hipStream_t st,
                  bool compact = false /* MI_DL_FLAG_CE_COMPACT: only the 4 pilot rows per port */,
                  const uint32_t* list = nullptr, uint32_t n_list = 0);
// equalise (combining the antennas) + soft demap + descramble (srslte_predecoding_* / demod_soft / scrambling_f)
void launch_demap(const float2* grid, const float2* ce, float* e, const MiSfDesc* sfs,
                  const MiPdschDesc* pd, const MiCellDesc* cells, const uint32_t* re_tab,
                  const uint32_t* scr, uint32_t n_sf, uint32_t max_units, float noise, const RxPlanes& rx,
                  hipStream_t st);
// two-layer spatial multiplexing (TM3 / TM4) detection + soft demap + descramble of both codewords of every pair
// (Plan::sm; sm_detect.hip).  Reads both antenna planes: the batch has rx.n == 2.
void launch_sm_detect(const float2* grid, const float2* ce, float* e, const MiSmDesc* sm, uint32_t n_pairs,
                      uint32_t max_nre, const uint32_t* re_tab, const uint32_t* scr, float noise, const RxPlanes& rx,
                      hipStream_t st);
// rate de-matching + HARQ combining into the group-interleaved softbuffer (srslte_rm_turbo_rx)
void launch_rm_combine(const float* e, float* sb, const MiGroupDesc* groups, const MiLaneDesc* lanes,
                       const MiKTab* ktabs, const uint32_t* ktab_data, uint32_t n_groups,
                       uint32_t max_ncb, const uint32_t* items, const uint4* recs /* Plan::rm_recs */, uint32_t n_busy,
                       uint32_t n_dbusy /* Plan::rm_dbusy */,
                       uint32_t n_items, hipStream_t st);
// demap fused into rate de-matching: LLRs computed from grid + ce inside the rm staging (no LLR stream)
void launch_rm_fused(const float2* grid, const float2* ce, const MiLaneSrc* lane_src, const uint32_t* re_tab,
                     const uint32_t* scr_tab, float noise, float* sb, const MiGroupDesc* groups, const MiLaneDesc* lanes,
                     const MiKTab* ktabs, const uint32_t* ktab_data, uint32_t n_groups, uint32_t max_ncb,
                     uint32_t unit_kind /* Qm + 8 TM2 common to all lanes, 0 = mixed */,
                     const uint32_t* items /* Plan::rm_items, NULL = every chunk */,
                     const uint4* recs /* Plan::rm_recs: the busy items' folded records */, uint32_t n_busy,
                     uint32_t n_dbusy /* Plan::rm_dbusy: the leading direct-group items */, uint32_t n_items,
                     bool compact_ce, const RxPlanes& rx, hipStream_t st);
// row maps and zero rows of Plan::rm_direct's groups (rm.hip rm_direct_map_kernel), before the combine launch
void launch_rm_direct_maps(float* sb, const uint32_t* ktab_data, const MiRmDirect* dgs, uint32_t ndg, hipStream_t st);
// ---- turbo decoder (srslte_tdec_*) ----
// per code block (lane index li) results
struct TdecOut {
  uint8_t* cb_bytes;        // [li][CB_BYTES_STRIDE] packed decisions
  uint32_t* its;            // iterations used
  uint32_t* crc_ok;         // CB CRC verdict of the last iteration
  uint32_t* tb_part;        // partial TB-CRC24A register (tb_kernel combines them)
  uint8_t* payload;         // packed decoder, PDSCH batches: payload bytes written in place (MiLaneDesc pay_st /
                            // pay_n), no code-block rows; nullptr = rows
};
// The turbo stage's buffers, built once per run (Engine::launch_turbo) and taken by every turbo launcher, which unpacks
// it into its kernels' individual __restrict__ pointer parameters
struct TdecBufs {
  const float* sb;          // softbuffer arena
  uint32_t* wm;             // window masks, WM_STRIDE per group (launch_rowmask writes them, the decoders read them)
  float* scratch;
  uint8_t* dec;
  TdecOut out;
  const MiGroupDesc* groups;
  const MiLaneDesc* lanes;
  const MiKTab* ktabs;
  const uint32_t* kdata;
};
// the waterfall continuation's buffers and their sizes
struct TdecContBufs {
  uint32_t* cont;           // the lists: 1 + lanes words; with rounds 3 n_groups * 64 + 2 (two lists and the sources)
  uint32_t* cscr;           // max_pairs x pair_u32 words: the dense pairs' state
  uint8_t* cdec;            // max_pairs x K x 64 decision bytes
  uint32_t max_pairs;
  size_t pair_u32;
  size_t scr_pair_u32;      // rounds: the stride of a group pair's own scratch, reused (with dec) as pair buffers
};
// and its schedule
struct TdecContSched {
  uint32_t gather_wgs;      // workgroups of the (grid-stride) gathers
  bool w_stored;            // the first launch stored w rows: gather them (no DEC2 re-run)
  bool rounds;              // one iteration per launch, the failing code blocks re-compacted between them
  uint32_t seg;             // rounds: 0, or the rounds after the first segmented over 4 / 8 wavefronts per pair
                            // (tdec_kernel_p2s)
  uint32_t* h_count;        // page-locked [CONT_HIST]: the code blocks each round decodes (round 1: those continuing
                            // after iteration 0); nullptr = not recorded
  bool cont_zeroed;         // cont[0] already reset on the stream (launch_rowmask's zero)
};
constexpr uint32_t CONT_HIST = 8;   // rounds whose counts are recorded (h_count)
// window masks of the sparse softbuffer rows (which decoder inputs have a materialised row); zero (if set) is reset
void launch_rowmask(const TdecBufs& b, uint32_t n_groups, uint32_t* zero, hipStream_t st);
// one wavefront per group of 64 code blocks
void launch_tdec(const TdecBufs& b, uint32_t n_groups, uint32_t max_its, uint32_t early_stop, bool q16,
                 int crossed /* 0 one wavefront per group, 1 crossed, 2 crossed recompute */, hipStream_t st);
// packed int16 decoder, two code blocks per lane: one workgroup (crossed wavefronts F and B) per group pair
// (Plan::pairs)
void launch_tdec_p2(const TdecBufs& b, const uint32_t* pairs, uint32_t n_pairs, uint32_t max_its, uint32_t early_stop,
                    bool no_w /* DEC2 stores no extrinsic rows (a one-iteration first launch, tdec_p2_body.h) */,
                    hipStream_t st);
// waterfall compaction after iteration 0 of launch_tdec_p2 (one K, early stop; tdec_p2_body.h P2ContSrc):
// gather the CRC-failing code blocks into dense continuation pairs and decode iterations 1 .. max_its - 1 there
bool launch_tdec_cont(const TdecBufs& b, const TdecContBufs& c, const TdecContSched& s, uint32_t n_groups,
                      const MiKTab& kt, uint32_t K, uint32_t max_its, hipStream_t st);
// latency form of the int16 turbo decoder: one workgroup of `threads` (64/128/256) per code block
// (lane descriptor), exact trellis segments (tdec_win_body.h); max_k sizes the dynamic LDS
void launch_tdec_win(const TdecBufs& b, uint32_t n_lanes, uint32_t max_k, uint32_t max_its, uint32_t early_stop,
                     uint32_t threads, hipStream_t st);
// raw code-block decoder input [cb][3(K+4)] -> group-interleaved softbuffer layout
void launch_cb_scatter(const float* d, float* sb, const MiGroupDesc* groups, const MiKTab* ktabs,
                       const uint32_t* kdata, uint32_t n_groups, uint32_t K, uint32_t n_cb, hipStream_t st);
// TB assembly + CRC24A + payload packing
void launch_tb(const uint8_t* cb_bytes, uint8_t* payload, uint32_t* tb_crc_ok, uint32_t* tb_its,
               const uint32_t* cb_its, const uint32_t* cb_tbp, const MiTbDesc* tbs, uint32_t n_tb,
               const uint32_t* cb_list, const uint32_t* kdata, bool copy /* false: payload already written */,
               hipStream_t st);

}  // namespace mi
