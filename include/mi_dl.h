/*
 * mi_dl.h -- batched MI355X LTE downlink PDSCH receiver (C ABI, no torch types).
 *
 * The batched extension SURVEY.md 8b asks for beside the per-TTI srsLTE API of
 * include/srslte/srslte.h: N subframes (IQ resident in HBM) are taken through
 *   OFDM RX -> CRS channel estimation -> equalisation -> soft demap -> descrambling ->
 *   rate de-matching + HARQ combining -> max-log-MAP turbo decoding -> TB CRC -> payload
 * by a fixed sequence of gfx950 kernels on one HIP stream.  The per-subframe work is what
 * srsUE's phch_worker performs per TTI through srslte_ue_dl_decode_fft_estimate and
 * srslte_pdsch_decode_rnti (/root/reference/ue/src/phy/phch_worker.cc:254, :347-348).
 *
 * Multi-GPU: one process per GPU, each with its own batch (subframes are independent; no
 * collective on the data path).  All functions return 0 on success and a negative value on
 * error, like the srsLTE API (SRSLTE_SUCCESS / SRSLTE_ERROR).
 */
#ifndef MI_DL_H
#define MI_DL_H
#include <stddef.h>
#include <stdint.h>

#include "srslte/common/timestamp.h"   /* srslte_timestamp_t of the receive callback (mi_acq_create) */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_DL_MAX_PRB 110

typedef struct {
  uint32_t cell_id;      /* N_ID^cell */
  uint32_t nof_prb;      /* 6, 15, 25, 50, 75, 100 */
  uint32_t nof_ports;    /* 1 or 2 CRS ports */
  uint32_t sf_idx;       /* 0..9 */
  uint32_t cfi;          /* 1..3 (control symbols) */
  uint32_t tm;           /* 1 = single port, 2 = transmit diversity (SFBC), 3 = open-loop spatial multiplexing
                          * (large-delay CDD), 4 = closed-loop spatial multiplexing: two layers, two codewords (below) */
  uint32_t nl_td;        /* N_L used by rate matching for TM2 (36.212 5.1.4.1.2: 2) */
  uint32_t rnti;
  uint32_t rv;           /* redundancy version 0..3 */
  uint32_t tbs;          /* transport block size, bits */
  uint32_t Qm;           /* 2, 4, 6 */
  uint32_t new_tb;       /* 1 = first transmission (softbuffer overwritten), 0 = HARQ combine */
  /* allocated PRBs.  If every entry is 0 or 1, a non-zero entry = PRB used in both slots (localized).
   * Otherwise bit 0 / bit 1 of entry p = PRB p used in slot 0 / slot 1 (distributed VRB, 36.211 6.2.3.2:
   * srslte_ra_dl_grant_t.prb_idx[0] / [1]); the RE gather follows 36.211 6.3.5 per slot. */
  uint8_t  prb_mask[MI_DL_MAX_PRB];
  /* Spatial multiplexing (tm 3 / 4; both 0 for tm 1 / 2, where a zeroed pair plans exactly as before the fields
   * existed).  A spatially multiplexed subframe -- 2 CRS ports, 2 receive antennas, 2 layers, one codeword per layer --
   * is TWO consecutive entries of the cfg array: entry i with cw = 0 and entry i + 1 with cw = 1, both with the same
   * cell, sf_idx, cfi, tm, pmi, rnti and prb_mask, each with its own tbs, Qm, rv and new_tb (nl_td is ignored:
   * N_L = 1 per codeword).  The cw = 1 entry is a transport block of its own everywhere after the LLRs (LLR range,
   * code blocks, softbuffer rows, payload, tb_crc, tb_its) but owns no samples: its IQ / grid / ce offsets are its
   * partner's, it adds nothing to mi_dl_batch_iq_samples or the grid / ce buffers, the front end runs once per
   * physical subframe and its MI_DL_BUF_METRICS row is never written. */
  uint32_t cw;           /* codeword q of the entry: 0 or 1 */
  uint32_t pmi;          /* tm 4: two-layer codebook index 1 or 2 (36.211 Table 6.3.4.2.3-1); ignored for tm 3 */
} mi_dl_sf_cfg_t;

/* stages, for mi_dl_batch_stage_ms */
enum { MI_DL_STAGE_OFDM = 0, MI_DL_STAGE_CHEST, MI_DL_STAGE_DEMAP, MI_DL_STAGE_RM, MI_DL_STAGE_TDEC,
       MI_DL_STAGE_TB, MI_DL_NSTAGES };

/* buffers that can be downloaded for parity checks */
enum { MI_DL_BUF_GRID = 0, MI_DL_BUF_CE, MI_DL_BUF_LLR, MI_DL_BUF_PAYLOAD, MI_DL_BUF_TB_CRC, MI_DL_BUF_TB_ITS,
       MI_DL_BUF_METRICS, MI_DL_BUF_CB_ITS, MI_DL_BUF_CB_CRC,
       MI_DL_BUF_SOFTBUFFER /* the batch's HARQ softbuffer arena (group layout, dl_common.h sb_group_floats) */ };

#define MI_DL_FLAG_PROFILE 1u  /* record HIP events around every stage of every run */
/* turbo decoder arithmetic.  Default (and MI_DL_FLAG_TDEC_I16): the int16 decoder of srsLTE's SSE
 * design (srslte_tdec_sse, what srsUE runs on SSE4.1 hosts: reference CMakeLists.txt:58-68 adds
 * -DLV_HAVE_SSE), fixed-point contract in DESIGN.md 4.5.  MI_DL_FLAG_TDEC_GEN: the float
 * srsLTE-gen decoder (srslte_tdec_gen, the non-SSE build).  Both are bit-exact to their oracle. */
#define MI_DL_FLAG_TDEC_I16 2u
#define MI_DL_FLAG_TDEC_GEN 4u
/* IQ input in UHD's sc16 wire format (int16 I/Q, fc32 = sc16 / 32768) instead of fc32: half the
 * bytes over PCIe for host-resident IQ; the OFDM stage converts on load (exact). */
#define MI_DL_FLAG_IQ_SC16 8u
/* turbo decoder schedule (int16 arithmetic only; results are identical either way).  Default: the
 * latency form (one workgroup per code block, exact trellis segments) when the batch
 * holds at most MI_TDEC_WIN_AUTO_CBS code blocks, else one code block per lane of 64-lane wavefronts.
 * MI_DL_FLAG_TDEC_WIN / MI_DL_FLAG_TDEC_LANE force one of them. */
#define MI_DL_FLAG_TDEC_WIN  16u
#define MI_DL_FLAG_TDEC_LANE 32u
#define MI_TDEC_WIN_AUTO_CBS 1024u
/* Keep the LLR stream (MI_DL_BUF_LLR) of a full run.  By default a run that includes both the DEMAP and
 * the RM stage fuses them: rate de-matching computes each LLR from the grid and channel estimates (the
 * same arithmetic, demap_body.h) and the LLR stream is never written.  Runs of RM without DEMAP read the
 * LLR buffer (e.g. uploaded by the caller). */
#define MI_DL_FLAG_KEEP_LLR  64u
/* Lane-per-code-block turbo decoder in the crossed schedule: two wavefronts per 64-code-block group, the
 * forward and backward recursions of each half-iteration run concurrently and meet in the middle
 * (bit-identical outputs, tdec_body.h).  Without MI_DL_FLAG_TDEC_X / MI_DL_FLAG_TDEC_LANE the int16 lane
 * form is always crossed (the float one below 2 groups per SIMD); MI_DL_FLAG_TDEC_LANE alone = one
 * wavefront per group. */
#define MI_DL_FLAG_TDEC_X    128u
/* with MI_DL_FLAG_TDEC_X: force the crossed kernel's recompute form (metric windows recomputed per step,
 * 92 VGPRs, 5 waves per SIMD; int16 decoder).  Default: chosen when the batch's wavefronts fit in one
 * round at 5 but not at 4 waves per SIMD. */
#define MI_DL_FLAG_TDEC_XR   256u
/* int16 decoder, lane form with TWO code blocks per lane: the trellis metrics of a code block of group A
 * (low 16 bits) and of the same lane of an equal-K group B (high 16 bits) in one register, advanced by
 * packed int16 instructions (half the VALU instructions per code block), crossed schedule; bit-identical
 * outputs (tdec_p2_body.h) */
#define MI_DL_FLAG_TDEC_P2   512u
/* compact channel estimates: the channel-estimation stage writes, per port, only the 4 pilot symbols'
 * frequency-interpolated rows ([port][4][12 N_RB] at the subframe's ce offset) and the fused demap stage
 * interpolates each RE's estimate in time from them with the chest kernel's own expression -- identical
 * LLRs, 10 of 14 rows of channel-estimate traffic written and read never.  Batch throughput mode: the
 * batch's ce buffer then does not hold the full estimates (no MI_DL_FLAG_KEEP_LLR, no mi_dl_ctrl_* on it; mi_dl_csi_*
 * reads either layout).
 * A run whose stage mask includes DEMAP but not CHEST after a compact estimation fails (returns -1,
 * mi_dl_last_error says why) instead of reading rows that were never written. */
#define MI_DL_FLAG_CE_COMPACT 1024u
/* waterfall compaction (packed decoder, CRC early stop): the re-compaction rounds after the first decode each dense
 * pair with 8 wavefronts, one per trellis segment, made exact by fix-up rounds instead of the crossed
 * pair of wavefronts: a shorter chain for more wavefronts.  Results identical.  Pays when the batch runs alone (one
 * stream, waterfall: +6 %); beside other streams' work the extra wavefronts cost more than the shorter chain saves
 * (4 streams: -2 %), so it is off by default. */
#define MI_DL_FLAG_TDEC_SEG  2048u

typedef struct mi_dl_batch mi_dl_batch_t;

/* Plans a batch (host work + device allocation, once).  max_its: turbo iteration cap
 * (srslte_sch_set_max_noi), early stop on the code-block CRC as srsLTE does. */
mi_dl_batch_t *mi_dl_batch_create(const mi_dl_sf_cfg_t *cfgs, uint32_t n_sf, uint32_t max_its, uint32_t flags);
/* Receive diversity: a batch of n_rx = 1 or 2 receive antennas (anything else returns NULL and sets
 * mi_last_error); mi_dl_batch_create is n_rx = 1.  With two antennas the front end (OFDM, channel estimation) runs
 * per antenna and the demap stage -- alone or fused into rate de-matching -- combines them per RE by maximum-ratio
 * combining: TM1 x = sum_a y_a h_a* / (sum_a |h_a|^2 + noise); TM2 the SFBC numerators and |h00|^2 + |h11|^2 summed
 * over the antennas.  Everything after the LLRs exists once.
 * Layout (antenna planes): the IQ, MI_DL_BUF_GRID, MI_DL_BUF_CE and MI_DL_BUF_METRICS buffers are n_rx consecutive
 * copies of the single-antenna buffer.  Antenna a of subframe i lives at mi_dl_batch_offset(b, which, i) +
 * a * mi_dl_batch_rx_stride(b, which) (the element units of mi_dl_batch_offset; 0 for single-plane buffers), its IQ at
 * sample mi_dl_batch_iq_offset(b, i) + a * mi_dl_batch_iq_rx_stride(b): a radio's per-channel receive buffers map
 * onto the planes directly.  mi_dl_batch_iq_samples stays one plane's samples; the d_iq of a run holds n_rx planes;
 * mi_dl_batch_bytes / _upload / _download / _device_ptr cover all planes.  The strides follow a re-plan.
 * MI_DL_FLAG_IQ_SC16, MI_DL_FLAG_CE_COMPACT and MI_DL_FLAG_KEEP_LLR work as with one antenna (the LLR stream is the
 * combined one).  mi_pbch_* and mi_dl_ctrl_create on a two-antenna batch read antenna 0 (plane 0); a control object
 * created with MI_CTRL_FLAG_RX_COMBINE combines both planes.  The per-TTI srslte_ue_dl_* API stays single-antenna.
 * Spatial multiplexing (tm 3 / 4 entry pairs, mi_dl_sf_cfg_t): only on a batch, pipe or re-plan with n_rx = 2 (else
 * NULL / -1 and mi_last_error).  The pair's two layers are detected per RE over both antennas,
 *   x^ = (G^H G + noise I)^-1 G^H y,  G = H P_i,  H[a][p] = antenna a's estimate of port p,  noise = 0.01,
 * P_i = (1/2) [[1, 1], [w, -w]] at RE i of the PDSCH mapping order with w = (-1)^i (tm 3), 1 / j (tm 4 pmi 1 / 2), then
 * demapped and descrambled per codeword (c_init with q 2^13) into the two entries' LLR ranges.  A run of a plan that
 * holds a pair is never fused: DEMAP writes the LLR stream and RM reads it, as with MI_DL_FLAG_KEEP_LLR, and
 * MI_DL_FLAG_CE_COMPACT is inert.  mi_dl_batch_iq_offset and mi_dl_batch_offset(GRID | CE) of a cw = 1 entry return its
 * partner's values; its MI_DL_BUF_METRICS row is never written.  TM1 / TM2 entries may share the batch. */
mi_dl_batch_t *mi_dl_batch_create_rx(const mi_dl_sf_cfg_t *cfgs, uint32_t n_sf, uint32_t n_rx, uint32_t max_its,
                                     uint32_t flags);
uint32_t mi_dl_batch_n_rx(const mi_dl_batch_t *b);
size_t mi_dl_batch_rx_stride(const mi_dl_batch_t *b, int which);
size_t mi_dl_batch_iq_rx_stride(const mi_dl_batch_t *b);
void   mi_dl_batch_destroy(mi_dl_batch_t *b);
/* IQ layout: subframe i starts at sample (cf32) mi_dl_batch_iq_offset(b, i) */
size_t mi_dl_batch_iq_offset(const mi_dl_batch_t *b, uint32_t sf);
size_t mi_dl_batch_iq_samples(const mi_dl_batch_t *b);
size_t mi_dl_batch_payload_offset(const mi_dl_batch_t *b, uint32_t sf);
size_t mi_dl_batch_bytes(const mi_dl_batch_t *b, int which);       /* size of a downloadable buffer */
size_t mi_dl_batch_offset(const mi_dl_batch_t *b, int which, uint32_t sf);  /* element offset per subframe */
/* Enqueue the whole receive chain on `stream` (a hipStream_t; NULL = default stream).
 * d_iq: device pointer to cf32 IQ, mi_dl_batch_iq_samples() samples.  Asynchronous. */
int    mi_dl_batch_run(mi_dl_batch_t *b, const void *d_iq, void *stream);
/* Run only the stages in stage_mask (bit i = MI_DL_STAGE_i) -- e.g. RM|TDEC|TB after
 * mi_dl_batch_upload(MI_DL_BUF_LLR) to decode given soft bits (parity tests). */
int    mi_dl_batch_run_stages(mi_dl_batch_t *b, const void *d_iq, void *stream, uint32_t stage_mask);
/* The whole chain with its front end (OFDM, channel estimation, demap + rate de-matching) on front_stream and its
 * back end (turbo decoding, TB CRC) on back_stream, ordered by events the batch owns: the back end waits for this
 * run's front end, and the batch's next run or re-plan (split or not, on any stream) waits for this back end (the
 * workspace is reused).  The run is complete when back_stream is; downloads synchronise it.  With the two streams on complementary CU shares
 * (mi_stream_create_cu_share) and several batches in flight, rate de-matching never shares a CU with the turbo
 * decoder: the headline step is 7.96-8.08 ms on every MI355X sampled, where whole runs on plain streams vary from
 * 7.86 to 8.35 ms by box.  front_stream == back_stream is mi_dl_batch_run.  Results are those of
 * mi_dl_batch_run. */
int    mi_dl_batch_run_split(mi_dl_batch_t *b, const void *d_iq, void *front_stream, void *back_stream);
/* Blocking copy of host data into a batch buffer (grid / ce / LLR injection for parity tests). */
int    mi_dl_batch_upload(mi_dl_batch_t *b, int which, const void *host, size_t bytes);
/* Blocking copy of a result buffer to host memory (synchronises the batch's last stream). */
int    mi_dl_batch_download(mi_dl_batch_t *b, int which, void *host, size_t bytes);
/* Device pointer of a result buffer (for zero-copy consumers). */
void  *mi_dl_batch_device_ptr(mi_dl_batch_t *b, int which);
/* Per-stage device time in ms, averaged over the runs since the last profile reset
 * (MI_DL_FLAG_PROFILE: HIP events recorded on the run's stream around every stage; synchronises). */
int    mi_dl_batch_stage_ms(mi_dl_batch_t *b, float *ms /* MI_DL_NSTAGES */, uint32_t *nruns);
void   mi_dl_batch_profile_reset(mi_dl_batch_t *b);
/* Algorithmic HBM bytes of one run (SURVEY.md 8d definitions) */
double mi_dl_batch_algo_bytes(const mi_dl_batch_t *b, int which_stage /* -1 = compulsory total */);
uint32_t mi_dl_batch_n_codeblocks(const mi_dl_batch_t *b);
/* turbo schedule of the batch: 1 = latency form (MI_DL_FLAG_TDEC_WIN rules), 2 = lane per code block in
 * the crossed schedule (two wavefronts per group), 3 = the same in its recompute form, 4 = two code blocks
 * per lane (packed int16, crossed), 0 = lane per code block, one wavefront per group */
int    mi_dl_batch_turbo_win(const mi_dl_batch_t *b);
/* 1 when schedule 4 runs with waterfall compaction: iteration 0 over every group pair, then the code blocks
 * whose CRC failed gathered into dense continuation pairs for the remaining iterations (early stop,
 * max_its > 1, one code-block size; the environment variable MI_TDEC_COMPACT=0 disables it for A/B runs) */
int    mi_dl_batch_turbo_compact(const mi_dl_batch_t *b);
uint32_t mi_dl_batch_n_groups(const mi_dl_batch_t *b);
/* groups whose rate de-matching runs in the direct form (every valid lane a new TB with one rank table, one
 * k0 rank, one modulation, E <= N_v: each LLR written straight to its softbuffer row); the others gather per
 * circular-buffer position.  The environment variable MI_RM_DIRECT=0 (read when the batch is created) disables
 * the direct form for A/B runs; the softbuffer is bit-identical either way. */
uint32_t mi_dl_batch_rm_direct_groups(const mi_dl_batch_t *b);
/* Waterfall compaction's schedule source.  With compaction the first launch chooses between two exact schedules
 * (store the iteration-0 extrinsic rows and re-compact per iteration, or not; and the size of the gather grid) from
 * the continuation counts of THIS batch's earlier runs, read back without a wait -- so by default the timing of a run
 * depends on the batch's history (its results never do).  mode: -1 = from the history (default); 0 = fixed "few
 * code blocks continue" (the high-SNR schedule); 1 = fixed "waterfall" (the low-SNR schedule).  A fixed mode makes
 * the schedule of every run a function of the call alone.  mi_dl_batch_reset_history forgets the recorded counts
 * (the next run of mode -1 schedules as a fresh batch). */
int    mi_dl_batch_set_tdec_history(mi_dl_batch_t *b, int mode);   /* 0 = ok, -1 = bad mode */
void   mi_dl_batch_reset_history(mi_dl_batch_t *b);

/* ---- streaming re-planning (srsUE re-derives the grant every TTI: phch_worker.cc:297 -> :337).
 * The planner is split from the device: mi_dl_plan_build runs the whole host planning of a batch (RE lists,
 * scrambling words, segmentation, 64-lane grouping, rate-matching work lists) with NO HIP call, so host
 * threads can plan step i+1 while the GPU decodes step i; mi_dl_batch_replan then swaps the built plan into a
 * batch and enqueues its table upload on `stream` -- ordered after the batch's earlier work on that stream,
 * so the caller passes the stream the batch runs on.  The plan object keeps its lookup caches (scrambling
 * words per (RNTI, sf, G), CRS per cell, per-K tables: srslte_ue_dl_set_rnti's pregeneration) across builds,
 * and after a replan it holds the batch's previous plan, ready to be rebuilt.  One plan object per planning
 * thread; a batch's work buffers only grow (a larger plan reallocates them, synchronously).
 * HARQ continuity across a replan, per 64-lane group: the softbuffer rows of a code block are where the plan puts
 * them, so soft combining (new_tb = 0 lanes) carries over for every group the new plan lays out exactly as the old
 * one did (same group index, K, N_cb, first lane and softbuffer offset, and the same code-block-to-lane assignment
 * in its 64 lanes -- e.g. the same grant with a new rv), whatever happens to the other groups.  A group whose layout
 * differs and that holds a retransmission lane has its softbuffer region cleared (every value RX_NULL, as
 * srslte_softbuffer_rx_reset), so such a lane combines with nothing rather than with another code block's rows --
 * srsLTE's softbuffer is per HARQ process, and a change of another subframe's grant does not touch it.  (New
 * transmissions overwrite their rows; rows another layout left are settled by the kernels.)  When the new plan needs a
 * larger softbuffer arena, the arena grows keeping its contents (a device copy; the new tail is RX_NULL), so the
 * unchanged groups keep combining across the growth too. */
typedef struct mi_dl_plan mi_dl_plan_t;
mi_dl_plan_t *mi_dl_plan_create(void);
void   mi_dl_plan_destroy(mi_dl_plan_t *p);
int    mi_dl_plan_build(mi_dl_plan_t *p, const mi_dl_sf_cfg_t *cfgs, uint32_t n_sf);   /* host only; 0 = ok */
int    mi_dl_batch_replan(mi_dl_batch_t *b, mi_dl_plan_t *p, void *stream);          /* 0 = ok */
/* HBM a batch holds: its work buffers, softbuffer arena, descriptor tables and twiddles (the LLR stream only once a
 * run or a buffer access needed it: the default fused demap never does).  mi_dl_plan_device_bytes: the work buffers
 * and softbuffer a batch of a built plan would allocate with these max_its / flags -- host only, no HIP call that
 * allocates; a deployer sizes workspaces per GPU with it (4 workspaces of 12,500 subframes). */
size_t mi_dl_batch_device_bytes(mi_dl_batch_t *b);
size_t mi_dl_plan_device_bytes(const mi_dl_plan_t *p, uint32_t max_its, uint32_t flags);
/* the same for a batch of n_rx receive antennas (0 and an error string for an n_rx other than 1 or 2) */
size_t mi_dl_plan_device_bytes_rx(const mi_dl_plan_t *p, uint32_t max_its, uint32_t flags, uint32_t n_rx);

/* ---- raw turbo code-block decoding (the srslte_tdec_* contract; BASELINE configs[0] =
 * srsLTE turbodecoder_test).  n_cb code blocks of size K; decoder input per block = 3(K+4) fp32
 * LLRs in triplet order d0_k d1_k d2_k with the 36.212 tail layout, LLR > 0 => bit 1 (device
 * memory, [n_cb][3(K+4)]).  max_its iterations; early_stop on the block CRC (24A if crc24a, else
 * 24B) or a fixed iteration count.  Decisions: K/8 bytes per block, MSB first. */
typedef struct mi_tdec_batch mi_tdec_batch_t;
mi_tdec_batch_t *mi_tdec_create(uint32_t K, uint32_t n_cb, uint32_t max_its, int early_stop, int crc24a,
                                uint32_t flags);
void   mi_tdec_destroy(mi_tdec_batch_t *b);
int    mi_tdec_run(mi_tdec_batch_t *b, const float *d_in, void *stream);
int    mi_tdec_download(mi_tdec_batch_t *b, uint8_t *bits /* n_cb*K/8 */, uint32_t *its, uint32_t *crc_ok);
int    mi_tdec_stage_ms(mi_tdec_batch_t *b, float *ms /* MI_DL_NSTAGES */, uint32_t *nruns);
void   mi_tdec_profile_reset(mi_tdec_batch_t *b);
double mi_tdec_algo_bytes(const mi_tdec_batch_t *b);
int    mi_tdec_turbo_win(const mi_tdec_batch_t *b);
/* 36.212 5.1.3 turbo encoder (host): bits[K] -> d[3(K+4)] triplet order, 2 = <NULL> filler */
int    mi_turbo_encode(const uint8_t *bits, uint32_t K, uint32_t F, uint8_t *d);

/* ---- synthetic transmitter (eNB side, host) used to build benchmark input ------------------
 * Mirrors srsLTE's PDSCH encode chain: CRC24A, segmentation, turbo code, rate matching,
 * scrambling, QAM, SFBC, RE mapping + CRS + PCFICH, IFFT (1/sqrt N) + CP, flat per-port
 * channel h and AWGN at snr_db per RE (>= 200 => noiseless).  iq: 2 * 15 N floats. */
int    mi_tx_subframe(const mi_dl_sf_cfg_t *cfg, const uint8_t *tb, const float *h_re_im /* 2*ports */,
                      float snr_db, uint64_t noise_seed, float *iq);
/* The same for a spatially multiplexed subframe (tm 3 / 4): cfg_pair = its cw 0 and cw 1 entries, tb0 / tb1 their
 * transport blocks.  Per-codeword scrambling (c_init with q 2^13), layer mapping x0 = d0, x1 = d1, precoding
 * [y_port0; y_port1] = P_i [x0; x1] with P_i = (1/2) [[1, 1], [w, -w]] at RE i of the PDSCH mapping order: w = (-1)^i
 * for tm 3 (W D(i) U, 36.211 6.3.4.2.2), 1 / j for tm 4 pmi 1 / 2 (6.3.4.2.3); CRS and PCFICH as mi_tx_subframe.  h: one
 * receive antenna's flat channel per port; call once per receive antenna (own h, own noise seed). */
int    mi_tx_subframe_sm(const mi_dl_sf_cfg_t *cfg_pair, const uint8_t *tb0, const uint8_t *tb1,
                         const float *h_re_im /* 2*2 */, float snr_db, uint64_t noise_seed, float *iq);
int    mi_sf_len(uint32_t nof_prb);
/* number of PDSCH bits G of a configuration (RE count x Qm, 36.211 6.3.5 / 6.4) */
int    mi_pdsch_G(const mi_dl_sf_cfg_t *cfg);

/* ---- DL control channels ----------------------------------------------
 * PCFICH -> CFI, PDCCH soft bits and DCI blind search (srslte_pdcch_extract_llr +
 * srslte_ue_dl_find_dl_dci / _find_ul_dci) over the grid and channel estimates a batch's front end
 * left in HBM.  Per subframe the search uses that subframe's cfg.rnti and cfg.cfi; PHICH resources
 * phich_ng = 0..3 (Ng = 1/6, 1/2, 1, 2; normal duration).  run() enqueues four kernels (stage mask:
 * 1 PCFICH, 2 PDCCH soft bits, 4 blind search, 8 PHICH); result() returns the first DCI of the
 * subframe in srsLTE's search order (one DCI size over all candidates of a space at a time): `ul` 0 =
 * DL for a C-RNTI (UE-specific L = 1, 2, 4, 8 with 1A then 1, common L = 4, 8 with 1A), 1 = UL format 0,
 * 2 = DL for an SI/RA/P-RNTI (common space only, 1A then 1C).  format: 0 = 0, 1 = 1, 2 = 1A, 3 = 1C (4 = 2, 5 = 2A
 * with MI_CTRL_FLAG_TM_FORMATS, below).
 * Returns 1 found, 0 not found, -1 error.  PHICH (srslte_ue_dl_decode_phich, phch_worker.cc:381): set_phich() sets per subframe the
 * UL grant's lowest PRB index and DMRS cyclic shift (36.213 9.1.2; default 0, 0), phich() returns the
 * HARQ indicator (1 ACK, 0 NACK, -1 error) and its soft value (> 0 favours ACK).
 *
 * mi_dl_ctrl_create_flags (flags = 0 is mi_dl_ctrl_create):
 *   MI_CTRL_FLAG_RX_COMBINE  two-antenna batch only (else NULL and mi_last_error): PCFICH, the PDCCH soft bits and PHICH
 *     combine both antenna planes per RE with the PDSCH demapper's maximum-ratio combining (mi_dl_batch_create_rx): one
 *     port x = sum_a y_a h_a* / (sum_a |h_a|^2 + noise); two ports the SFBC numerators and |h00|^2 + |h11|^2 summed over
 *     the antennas (the one-port PHICH floors the summed denominator at 1e-9).  The blind search reads the combined
 *     soft bits.  Without the flag a two-antenna batch's control object reads plane 0, as before.
 *   MI_CTRL_FLAG_TM_FORMATS  the second DCI size of the UE-specific space follows the entry's tm: tm 1 / 2 format 1, tm 3
 *     format 2A, tm 4 format 2 (2 CRS ports; 36.212 5.3.3.1.5 / 5.3.3.1.5A), so the search order for ul = 0 is the 1A
 *     size, then that format, then the common space's 1A size, and the job count per subframe does not grow.  result()
 *     reports format 4 = format 2 and 5 = format 2A (unpack with mi_dci_dl2_unpack).  The cw = 1 entry of a codeword pair
 *     owns no samples: it gets no jobs, and result / n_cce / llr_offset / phich on it report its partner's.  Without the
 *     flag a pair's two entries are searched as two format 1 subframes, as before.
 * mi_dl_ctrl_n_jobs: the (candidate, size) decodes of one run. */
#define MI_CTRL_FLAG_RX_COMBINE 1u
#define MI_CTRL_FLAG_TM_FORMATS 2u
typedef struct mi_dl_ctrl mi_dl_ctrl_t;
mi_dl_ctrl_t *mi_dl_ctrl_create(mi_dl_batch_t *b, uint32_t phich_ng);
mi_dl_ctrl_t *mi_dl_ctrl_create_flags(mi_dl_batch_t *b, uint32_t phich_ng, uint32_t flags);
uint32_t      mi_dl_ctrl_n_jobs(const mi_dl_ctrl_t *c);
void          mi_dl_ctrl_destroy(mi_dl_ctrl_t *c);
int           mi_dl_ctrl_run(mi_dl_ctrl_t *c, void *stream);
int           mi_dl_ctrl_run_stages(mi_dl_ctrl_t *c, uint32_t mask, void *stream);
int           mi_dl_ctrl_result(mi_dl_ctrl_t *c, uint32_t sf, int ul, uint32_t *cfi, uint32_t *format, uint32_t *L,
                                uint32_t *ncce, uint8_t *bits /* 64 */, uint32_t *nbits);
size_t        mi_dl_ctrl_llr_floats(const mi_dl_ctrl_t *c);
size_t        mi_dl_ctrl_llr_offset(const mi_dl_ctrl_t *c, uint32_t sf);
uint32_t      mi_dl_ctrl_n_cce(const mi_dl_ctrl_t *c, uint32_t sf);
/* copy PDCCH soft bits between host and device (upload != 0: host -> device) */
int           mi_dl_ctrl_llr(mi_dl_ctrl_t *c, float *host, size_t n, int upload);
int           mi_dl_ctrl_set_phich(mi_dl_ctrl_t *c, const uint32_t *i_lowest, const uint32_t *n_dmrs);
int           mi_dl_ctrl_phich(mi_dl_ctrl_t *c, uint32_t sf, float *soft);

/* ---- DCI formats 2 / 2A: the grants of TM4 / TM3 (36.212 5.3.3.1.5 / 5.3.3.1.5A; host only, no device) ----------
 * FDD, 2 CRS ports (any other port count is rejected: -1 and mi_last_error).  Field order: [resource allocation header
 * if N_RB > 10], ceil(N_RB / P) resource-block assignment bits (type 0: RBG bitmap; type 1: subset, shift, bitmap:
 * 36.213 7.1.6.1 / 7.1.6.2), TPC 2, HARQ process 3, TB-to-codeword swap 1, TB 1 (MCS 5, NDI 1, RV 2), TB 2 likewise,
 * precoding information 3 (format 2) / 0 (format 2A); one zero bit appended when the size is one of Table 5.3.3.1.2-1.
 * Sizes at 6 / 15 / 25 / 50 / 75 / 100 PRB: format 2: 31 34 39 43 45 51; format 2A: 28 31 36 41 42 48.  Bits are one per
 * byte, as mi_dl_ctrl_result returns them.
 * mi_dci_dl2_to_cfg turns an unpacked grant into the batch entries that decode it.  base: cell_id, nof_prb, nof_ports,
 * sf_idx, cfi and rnti of the subframe.  new_tb[t]: the caller's HARQ entity's verdict on TB t's NDI (MAC is out of
 * scope).  reported_cb_r2: the rank-2 codebook index the UE last reported (mi_dl_csi_result_t.cb_r2), used when the
 * precoding information says "as reported".  prb_mask from the type 0 / type 1 assignment; per enabled TB, tbs / Qm from
 * the MCS at the allocation's PRB count (one layer per codeword), rv from the DCI.  TB-to-codeword mapping of Tables
 * 5.3.3.1.5-1 / -2: the swap flag with both TBs enabled, a single enabled TB on codeword 0.  Both TBs enabled: format 2A
 * a tm = 3 pair; format 2 a tm = 4 pair with pmi 1 / 2 for pinfo 0 / 1, pmi = reported_cb_r2 for pinfo 2 (-1 unless that
 * is 1 or 2), -1 for pinfo 3..7.  One TB enabled: format 2A, or format 2 with pinfo 0 (transmit diversity): one tm = 2
 * entry (nl_td = 2, cw = pmi = 0); format 2 with pinfo 1..6 (rank-1 closed-loop precoding, not built): -1.  MCS 29..31:
 * -1.  Writes 1 or 2 entries and returns that number; every -1 leaves out untouched. */
enum { MI_DCI_2 = 4, MI_DCI_2A = 5 };
typedef struct {
  uint32_t format, alloc_type;                 /* alloc_type 0 / 1 (36.213 7.1.6.1 / 7.1.6.2) */
  uint32_t type0_alloc;                        /* RBG bitmap, MSB = RBG 0 */
  uint32_t type1_subset, type1_shift, type1_bitmap;
  uint32_t tpc_pucch, harq_process, tb_cw_swap;
  struct { uint32_t mcs, ndi, rv, enabled; } tb[2];   /* enabled = !(mcs == 0 && rv == 1) */
  uint32_t pinfo;                              /* format 2: the 3 precoding-information bits; 2A with 2 ports: 0 */
} mi_dci_dl2_t;
int mi_dci_dl2_size(uint32_t format, uint32_t nof_prb, uint32_t nof_ports);          /* bits, -1 */
int mi_dci_dl2_pack(uint32_t nof_prb, uint32_t nof_ports, const mi_dci_dl2_t *d, uint8_t bits[64]);   /* bit count, -1 */
int mi_dci_dl2_unpack(uint32_t format, uint32_t nof_prb, uint32_t nof_ports, const uint8_t *bits, uint32_t nbits,
                      mi_dci_dl2_t *d);                                               /* 0, -1 */
int mi_dci_dl2_to_cfg(const mi_dci_dl2_t *d, const mi_dl_sf_cfg_t *base, const uint8_t new_tb[2],
                      uint32_t reported_cb_r2, mi_dl_sf_cfg_t out[2]);

/* ---- CSI feedback: CQI, PMI and RI from the channel estimates -------------------
 * What the UE reports so that an eNB can schedule TM4 with a precoder or TM3 / TM4 with two layers, computed over the
 * channel estimates a batch's CHEST stage left in HBM (one kernel, one workgroup per physical subframe; the default
 * batch run does not launch it).  Sample points: every subcarrier of the four CRS symbols 0, 4, 7, 11 -- the rows a
 * MI_DL_FLAG_CE_COMPACT run keeps, so run() follows whichever layout (full or compact) the batch's last CHEST stage
 * wrote.  Noise n of a subframe: the mean over the batch's antennas of its chest metric [3] (noise_estimate), or the
 * value given with set_noise; either floored at 1e-9.  h_ap = antenna a's estimate of CRS port p.  Hypotheses (per-layer
 * SINR g at a point):
 *   MI_CSI_H_BASE      one port: sum_a |h_a0|^2 / n; two ports (transmit diversity): sum_a (|h_a0|^2 + |h_a1|^2) / (2 n)
 *   MI_CSI_H_R1 + i    rank 1 closed loop, codebook index i = 0..3 (36.211 Table 6.3.4.2.3-1): W = (1/sqrt 2) [1, q]^T,
 *                      q = 1, -1, j, -j;  g = sum_a |h_a0 + q h_a1|^2 / (2 n)
 *   MI_CSI_H_R2 + 0/1  rank 2 closed loop, codebook index 1 / 2: G = H P, P = (1/2) [[1, 1], [w, -w]], w = 1 / j; per-layer
 *                      MMSE SINR g_l = 1 / [(I + G^H G / n)^-1]_ll - 1
 *   MI_CSI_H_CDD       rank 2 open loop (TM3, w alternating +1 / -1): both layers (cap[R2 + 0][0] + cap[R2 + 0][1]) / 2
 * cap[band][h][layer] = mean over the band's points of log2(1 + g) (rank-1 hypotheses: layer 0 only); band 0 = the whole
 * bandwidth, bands 1..n_sb = the higher-layer-configured subbands of 36.213 Table 7.2.1-3 (mi_csi_subbands: 4 / 6 / 8 PRB
 * for 8..26 / 27..63 / 64..110 PRB, none below 8, the last subband takes the remaining PRBs).  cqi[band][h][layer] =
 * srslte_cqi_from_snr(10 log10(2^cap - 1)).  Decisions, from the wideband capacities, ties to the lower index:
 * pmi_r1 = argmax_i cap[0][R1 + i][0]; cb_r2 = 1 or 2 = argmax of the two layers' sum; ri_cl = 2 if that sum exceeds
 * the best rank-1 capacity, else 1; ri_ol = 2 if 2 cap[0][CDD][0] > cap[0][BASE][0], else 1.  Evaluated (valid_mask bit
 * h; the other cells are 0, the decisions of missing hypotheses 0 / rank 1): one port: BASE; two ports, one antenna:
 * BASE and R1; two ports, two antennas: all.
 * The object describes the plan its batch held at create(), like mi_dl_ctrl_*: after mi_dl_batch_replan create a new
 * one (run() returns -1 when the batch's layout no longer matches).  The cw = 1 entry of a spatial multiplexing pair
 * reports its partner's record.  On a two-antenna batch CSI combines both planes.
 * run(): asynchronous, on `stream`; the caller orders it after the batch's CHEST stage (same stream, or an event) and
 * before the batch's next run.  -1 before any CHEST stage (or MI_DL_BUF_CE upload) of the batch.  set_noise(): one
 * value per batch entry (copied; synchronises), NULL = the chest metrics again (the default).  result() / download()
 * synchronise run()'s stream; download() copies all mi_dl_csi_n(c) records.  device_ptr(): the records in HBM.
 * mi_csi_pack_pucch: the PUCCH format 2 payload for 2 ports (36.212 Tables 5.2.3.3.1-1 / -2), bits MSB first, one per
 * byte (as srslte_cqi_value_pack; fits MI_PUCCH_UCI and mi_ul_cfg_t.cqi): tm 1 / 2 / 3: the 4-bit wideband CQI of
 * BASE (of CDD when tm 3 and ri_ol = 2); tm 4, ri_cl = 1: CQI (4) + PMI (2) = 6 bits; tm 4, ri_cl = 2: codeword 0's
 * CQI (4) + spatial differential CQI (3, 36.213 Table 7.2-2: offset = CQI0 - CQI1; 0, 1, 2, >= 3 -> 0, 1, 2, 3 and
 * <= -4, -3, -2, -1 -> 4, 5, 6, 7) + PMI (1 = cb_r2 - 1) = 8 bits.  Returns the bit count (*ri = the rank reported
 * with it), -1 on a bad argument or a report whose hypotheses the record does not hold. */
#define MI_CSI_NHYP   8
#define MI_CSI_MAX_SB 14
enum { MI_CSI_H_BASE = 0, MI_CSI_H_R1 = 1, MI_CSI_H_CDD = 5, MI_CSI_H_R2 = 6 };
typedef struct {
  uint32_t valid_mask;          /* bit h: hypothesis h was evaluated */
  uint32_t n_sb, sb_prb;        /* subbands and their size in PRB (0, 0: none) */
  uint32_t pmi_r1;              /* best rank-1 codebook index 0..3 */
  uint32_t cb_r2;               /* best rank-2 codebook index 1 or 2 (0: not evaluated) */
  uint32_t ri_cl, ri_ol;        /* rank 1 or 2, closed loop (TM4) and open loop (TM3) */
  float    noise;               /* the n used */
  float    cap[1 + MI_CSI_MAX_SB][MI_CSI_NHYP][2];
  uint8_t  cqi[1 + MI_CSI_MAX_SB][MI_CSI_NHYP][2];
} mi_dl_csi_result_t;
typedef struct mi_dl_csi mi_dl_csi_t;
mi_dl_csi_t *mi_dl_csi_create(mi_dl_batch_t *b);
void         mi_dl_csi_destroy(mi_dl_csi_t *c);
uint32_t     mi_dl_csi_n(const mi_dl_csi_t *c);   /* records = entries of the batch */
int          mi_dl_csi_set_noise(mi_dl_csi_t *c, const float *per_sf_or_NULL);
int          mi_dl_csi_run(mi_dl_csi_t *c, void *stream);
int          mi_dl_csi_result(mi_dl_csi_t *c, uint32_t sf, mi_dl_csi_result_t *out);
int          mi_dl_csi_download(mi_dl_csi_t *c, mi_dl_csi_result_t *out /* mi_dl_csi_n(c) */);
void        *mi_dl_csi_device_ptr(mi_dl_csi_t *c);
/* host only */
int          mi_csi_subbands(uint32_t nof_prb, uint32_t *sb_prb, uint32_t *n_sb);   /* -1: nof_prb outside 6..110 */
int          mi_csi_pack_pucch(uint32_t tm, const mi_dl_csi_result_t *r, uint8_t bits[11], uint32_t *ri);

/* ---- sync front end ----------------------------------------------------
 * The data-parallel part of srslte_ue_sync_zerocopy (phch_recv.cc:321): PSS timing + N_ID_2 search,
 * the PSS CFO estimate, SSS detection (N_ID_1, subframe 0 or 5) and CFO correction, batched over
 * device-resident IQ (cf32 offsets in samples).  pss(): window i starts at d_iq[off[i]], candidate
 * lags 0..nlag-1 (the PSS symbol's useful part, N samples, starting at the lag), N_ID_2 candidates in
 * nid2_mask (bit u); rho = |sum x conj(p)|^2 / (E_x E_p); cfo in subcarrier spacings (|cfo| < 1).
 * sss(): subframe i starts at d_iq[sf_off[i]].  correct(): len samples of d_src[src_off[i]] rotated
 * by exp(-j 2 pi cfo[i] n / N) into d_dst[dst_off[i]] (enqueued on stream); pss / sss are synchronous.
 * mi_tx_sync adds the PSS / SSS of subframes 0 and 5 to a subframe's IQ (synthetic transmitter). */
typedef struct mi_sync mi_sync_t;
typedef struct { uint32_t nid2, lag; float rho, cfo; } mi_pss_result_t;
typedef struct { uint32_t nid1, sf5; float score; } mi_sss_result_t;
mi_sync_t *mi_sync_create(uint32_t nof_prb);
void       mi_sync_destroy(mi_sync_t *s);
uint32_t   mi_sync_fft_size(const mi_sync_t *s);
int        mi_sync_pss(mi_sync_t *s, const void *d_iq, const uint64_t *off, uint32_t n, uint32_t nlag,
                       uint32_t nid2_mask, mi_pss_result_t *out, void *stream);
int        mi_sync_sss(mi_sync_t *s, const void *d_iq, const uint64_t *sf_off, const uint32_t *nid2, const float *cfo,
                       uint32_t n, mi_sss_result_t *out, void *stream);
int        mi_sync_correct(mi_sync_t *s, const void *d_src, const uint64_t *src_off, void *d_dst,
                           const uint64_t *dst_off, const float *cfo, uint32_t n, uint32_t len, void *stream);
int        mi_tx_sync(uint32_t cell_id, uint32_t nof_prb, uint32_t sf_idx, float amp, float *iq);

/* ---- cell acquisition: PBCH / MIB decoding and cell search ----------------------------------
 * What srsUE reaches through srslte_ue_mib_decode and srslte_ue_cellsearch_scan (phch_recv.cc:137-253), batched.
 * Normal CP; cells with 1 or 2 CRS ports (a 4-port cell's MIB is reported as not found).
 *
 * PBCH (36.211 6.6, 36.212 5.3.1) over the grid and channel estimates a batch's front end (stages OFDM | CHEST)
 * left in HBM, like mi_dl_ctrl_*.  Every subframe of the batch with sf_idx 0 is one PBCH frame (frame_of():
 * its index, -1 for other subframes); any nof_prb.  run() enqueues up to two kernels (stage mask: 1 = soft
 * bits, 2 = decode).  Stage 1 writes per frame and port hypothesis (0 = 1 port, 1 = 2 ports: SFBC, only where
 * the subframe's cfg has nof_ports = 2) the 480 QPSK soft bits, not descrambled, at float
 * (2 frame + hypothesis) * 480 of the soft-bit buffer.  Stage 2 decodes candidates: candidate c is n_frames[c]
 * (1..4) consecutive radio frames of one cell given as batch subframe indices sf[4 c ..], oldest first.  For
 * each it tries, in this order, f = 1..n_frames newest frames combined, then 1 port before 2, then the 40 ms
 * phase of the newest frame sfn_offset = f-1..3 (at most 20 decodes), and reports the first whose CRC16 matches
 * the port count's mask: found, nof_ports, sfn_offset, n_frames_used and the 24 MIB bits (unpack with
 * srslte_pbch_mib_unpack; the newest frame's SFN is the unpacked sfn + sfn_offset).  set_candidates() checks
 * every index (inside the batch, a subframe 0, one cell per candidate) and returns -1 before anything is
 * launched; it leaves no candidates behind then.  result(): 1 found, 0 not found, -1 error.
 * mi_pbch_re_indices: the 240 PBCH REs of a cell in mapping order (grid index l * 12 nof_prb + k), host only.
 * mi_tx_pbch adds the PBCH quarter `phase` (0..3) of a BCH TTI carrying bch_payload to a subframe-0 IQ buffer
 * (synthetic transmitter: nof_ports 1 or 2, flat per-port channel h, NULL = (1, 0); OFDM scaling of
 * mi_tx_subframe, which leaves these REs empty). */
typedef struct mi_pbch mi_pbch_t;
typedef struct { uint32_t found, nof_ports, sfn_offset, n_frames_used; uint8_t bits[24]; } mi_pbch_result_t;
int        mi_pbch_re_indices(uint32_t cell_id, uint32_t nof_prb, uint32_t re[240]);
mi_pbch_t *mi_pbch_create(mi_dl_batch_t *b);
void       mi_pbch_destroy(mi_pbch_t *p);
uint32_t   mi_pbch_n_frames(const mi_pbch_t *p);
int        mi_pbch_frame_of(const mi_pbch_t *p, uint32_t sf);
int        mi_pbch_set_candidates(mi_pbch_t *p, const uint32_t *sf /* 4 per candidate */, const uint32_t *n_frames,
                                  uint32_t n_cand);
uint32_t   mi_pbch_n_jobs(const mi_pbch_t *p);   /* decodes the next run's stage 2 launches */
int        mi_pbch_run(mi_pbch_t *p, uint32_t mask, void *stream);
int        mi_pbch_result(mi_pbch_t *p, uint32_t cand, mi_pbch_result_t *out);
size_t     mi_pbch_llr_floats(const mi_pbch_t *p);
/* copy PBCH soft bits between host and device (upload != 0: host -> device) */
int        mi_pbch_llr(mi_pbch_t *p, float *host, size_t n, int upload);
int        mi_tx_pbch(uint32_t cell_id, uint32_t nof_prb, uint32_t nof_ports, const uint8_t bch_payload[24],
                      uint32_t phase, const float *h_re_im, float *iq);

/* Cell search over device-resident IQ at 1.92 Msps (6 PRB, N = 128; offsets in cf32 samples).  Window i is the
 * 9600 + 128 samples at d_iq[off[i]] (5 ms and one symbol): every lag 0..9599 is correlated with each of the
 * three PSS roots in chunks of 64 lags (one launch), and at each (window, root) peak the SSS is detected with
 * the peak's CFO estimate (one launch) -- where its symbol lies inside the window (peak lag >= 137).  out[u]
 * reports N_ID_2 = u over the windows, mirroring srslte_ue_cellsearch_result_t: cell_id = the most frequent
 * 3 N_ID_1 + u (ties: the higher mean peak), mode = its share of the windows, peak = mean rho of the agreeing
 * windows, psr = mean of peak / largest chunk maximum at least two chunks away from the peak's, cfo = mean
 * estimate in subcarrier spacings, sf_start = stream offset of a subframe-0 boundary (the last one at or
 * before the PSS's subframe of the newest agreeing window, plus whole frames if that lies before sample 0),
 * found = peak > threshold.  threshold <= 0 selects MI_CELLSEARCH_THRESHOLD: rho of noise alone over N = 128
 * samples is Beta(1, 127), so the chance that any of 3 x 9600 lags exceeds 0.2 is 28800 x 0.8^127 < 1e-7 per
 * window, while a cell at 0 dB per RE gives rho near 0.3 (ue_sync.cpp's floor of 0.01 for a known cell lies
 * inside the noise of a 128-sample window: the mean of Beta(1, 127) is 1/128).  Synchronous. */
#define MI_CELLSEARCH_THRESHOLD 0.2f
typedef struct mi_cellsearch mi_cellsearch_t;
typedef struct { uint32_t found, cell_id; float mode, peak, psr, cfo; uint64_t sf_start; } mi_cell_result_t;
mi_cellsearch_t *mi_cellsearch_create(void);
void       mi_cellsearch_destroy(mi_cellsearch_t *s);
int        mi_cellsearch_run(mi_cellsearch_t *s, const void *d_iq, const uint64_t *off, uint32_t n_windows,
                             float threshold, mi_cell_result_t out[3], void *stream);

/* Streaming acquisition over a receive callback at 1.92 Msps (the callback of srslte_ue_sync_init: it fills
 * nsamples cf32 and returns their number).  One instance per thread; the kernels and transfers of search() and
 * mib() run on the instance's own stream (the table uploads when an instance or its internal batch is created
 * are blocking copies).  search(): reads n_half_frames * 9600 + 128 samples, runs the cell search above
 * over them (sf_start counts samples since the instance was created) and consumes n_half_frames * 9600 of
 * them; returns the number of cells found (0..3, *best = the found N_ID_2 with the highest peak) or -1.
 * mib(): finds the cell's subframe 0 (PSS of cell_id mod 3 over a half frame, SSS check, as srslte_ue_sync's
 * find; up to 8 half frames), then per radio frame reads that subframe, removes the CFO (`cfo` in subcarrier
 * spacings, as search() reports it), runs OFDM + channel estimation on an internal 6-PRB 2-port slot, keeps the
 * last four frames' soft bits and decodes the growing candidate (1, 2, 3, 4 frames); stops at the first MIB
 * found or after max_frames.  Returns 1 found, 0 not found, -1 error.  mi_mib_t: the unpacked MIB, the port
 * count from the CRC mask, the 10-bit SFN of the frame it stopped on, that frame's subframe-0 stream index and
 * how many frames were read.  The frame timing is not tracked between frames (acquisition takes a few frames). */
typedef struct mi_acq mi_acq_t;
typedef struct {
  uint32_t nof_prb, nof_ports, phich_length, phich_resources, sfn, n_frames;
  uint64_t sf_start;
  uint8_t  bits[24];
} mi_mib_t;
mi_acq_t  *mi_acq_create(int (*recv)(void *, void *, uint32_t, srslte_timestamp_t *), void *handler);
void       mi_acq_destroy(mi_acq_t *a);
int        mi_acq_search(mi_acq_t *a, uint32_t n_half_frames, float threshold, mi_cell_result_t out[3], uint32_t *best);
int        mi_acq_mib(mi_acq_t *a, uint32_t cell_id, float cfo, uint32_t max_frames, mi_mib_t *mib);

/* ---- host-IQ streaming pipeline -------------------------------------
 * Double buffering for IQ that arrives in host memory (srsUE's sync thread writes the worker's
 * buffer, phch_recv.cc:321-322): two batches of the same configuration, one copy stream and one
 * compute stream.  submit() enqueues the H2D copy of host_iq (mi_dl_batch_iq_samples cf32, or sc16
 * with MI_DL_FLAG_IQ_SC16, batch
 * layout; pinned memory from mi_host_alloc for full PCIe rate) into the free slot behind that
 * slot's previous decode, then the decode behind the copy, and returns the slot (0/1) without
 * blocking: the copy of one batch overlaps the decode of the other.  wait() blocks until the slot's
 * decode is done; its outputs (mi_dl_pipe_batch + mi_dl_batch_download/device_ptr) stay valid
 * until the slot is submitted again, i.e. for one further submit(). */
typedef struct mi_dl_pipe mi_dl_pipe_t;
mi_dl_pipe_t  *mi_dl_pipe_create(const mi_dl_sf_cfg_t *cfgs, uint32_t n_sf, uint32_t max_its, uint32_t flags);
/* two slots of n_rx-antenna batches (mi_dl_batch_create_rx): submit() copies the n_rx IQ planes of host_iq */
mi_dl_pipe_t  *mi_dl_pipe_create_rx(const mi_dl_sf_cfg_t *cfgs, uint32_t n_sf, uint32_t n_rx, uint32_t max_its,
                                    uint32_t flags);
void           mi_dl_pipe_destroy(mi_dl_pipe_t *p);
int            mi_dl_pipe_submit(mi_dl_pipe_t *p, const void *host_iq);   /* slot, or -1 */
int            mi_dl_pipe_wait(mi_dl_pipe_t *p, int slot);
mi_dl_batch_t *mi_dl_pipe_batch(mi_dl_pipe_t *p, int slot);
/* page-locked host memory (hipHostMalloc) for IQ buffers */
void  *mi_host_alloc(size_t bytes);
void   mi_host_free(void *p);

/* ---- device / runtime helpers ------------------------------------------------------------ */
int    mi_device_count(void);
int    mi_set_device(int dev);
const char *mi_last_error(void);
/* A stream of the current device restricted to a share of its compute units (hipExtStreamCreateWithCUMask): CU i
 * belongs to the share when i mod 8 lies in [first, first + count), so a share spans every XCD; count = 8 gives a
 * plain non-blocking stream on all CUs.  (A masked stream is a blocking stream: it orders with the null stream.)
 * Release with mi_stream_destroy. */
int    mi_stream_create_cu_share(uint32_t first, uint32_t count, void **stream);
int    mi_stream_destroy(void *stream);

#ifdef __cplusplus
}
#endif
#endif
