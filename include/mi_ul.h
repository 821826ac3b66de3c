/*
 * mi_ul.h -- batched C ABI of the MI355X UL PUSCH transmit path.
 *
 * The per-TTI srsLTE entry points srsUE calls (srslte_ue_ul_cfg_grant + srslte_ue_ul_pusch_encode_
 * rnti_softbuffer, /root/reference/ue/src/phy/phch_worker.cc:551-560) are in srslte/srslte.h; this is
 * the throughput form: N PUSCH transmissions planned once, encoded per call on the caller's stream
 * from device-resident TB payloads into device-resident SC-FDMA IQ.
 *
 * Chain (gfx950 kernels, srsue_amd/csrc/ul.hip): TB CRC24A -> segmentation + CRC24B -> turbo encoder
 * (36.212 5.1.3.2, chunk-parallel recursive encoders) -> rate matching (5.1.4.1, full circular buffer)
 * -> channel interleaver (5.2.2.8, no UCI) -> scrambling (36.211 5.3.1) -> modulation (7.1) ->
 * transform precoding (5.3.3, mixed-radix DFT of M = 12 L_prb) -> mapping (5.3.4, per-slot PRBs) +
 * DMRS (5.5.2.1; L_prb 1, 2: the tabulated base sequences of 5.5.1.2) -> SC-FDMA (5.6: N-point transform, half-subcarrier shift, CP).
 * Uplink control information is multiplexed as 36.212 5.2.2.6-5.2.2.8 prescribe: CQI (O <= 11 bits: the
 * (32, O) block code; O > 11: CRC8 + tail-biting convolutional code) ahead of the data in the multiplexed
 * sequence, RI (1 or 2 bits) in the interleaver columns next to the HARQ-ACK ones (rate matching of the
 * data around both), HARQ-ACK (1 or 2 bits) puncturing the data next to the DMRS.
 * Normalisation: unit average power per used subcarrier (1/sqrt(M) DFT, 1/sqrt(N) IDFT).
 *
 * PUCCH (36.211 5.4 / 5.5.2.2, srsue_amd/csrc/pucch.hip): formats 1/1a/1b and 2/2a/2b, the second half of this
 * header.  mi_pucch_resource derives the resource (PRBs, sequence group, n', orthogonal cover and the cyclic
 * shift of every symbol), mi_pucch_select picks format and resource for a UCI combination (36.213 10.1, FDD),
 * mi_pucch_batch_* plans N transmissions once and encodes them per call from one device word of UCI each
 * into device-resident SC-FDMA IQ with the layout and normalisation of the PUSCH batch.  Limits: normal CP,
 * FDD, CQI payloads of A <= 11 bits (the (20, A) code's columns 0..10), no SPS resources, no format 3.
 *
 * PRACH (36.211 5.7, srsue_amd/csrc/prach.hip): the preamble of formats 0-3, the last part of this header.
 * mi_prach_resource derives format, lengths, physical root, cyclic shift and frequency position of one preamble of
 * a cell (unrestricted and restricted sets), mi_prach_send_tti is the timing of Table 5.7.1-2, mi_prach_batch_*
 * plans N preambles once and generates them per call into device-resident IQ at the UL sample rate, with an optional
 * frequency shift and scale per transmission.  Limits: FDD, formats 0-3 (no format 4), no power ramping.
 *
 * SRS (36.211 5.5.3, srsue_amd/csrc/srs.hip): the periodic sounding reference signal.  mi_srs_resource derives the
 * bandwidth, the frequency position (with frequency hopping), the base sequence and the cyclic shift of one
 * transmission, mi_srs_batch_* plans N transmissions once and encodes them per call into device-resident SC-FDMA IQ
 * with the layout and normalisation of the PUSCH batch: symbols 0..12 zero, the SRS in symbol 13.  Limits: FDD,
 * normal CP, one antenna port, no aperiodic SRS.
 *
 * PUSCH in SRS subframes (36.211 5.3.4, 36.212 5.2.2.6-5.2.2.8): mi_ul_cfg_t.n_srs = 1 shortens the transmission to 11
 * data symbols (rate matching, UCI multiplexing and an 11-column channel interleaver follow; symbol 13 is written as
 * zeros), n_symb_initial carries the first transmission's symbol count into a retransmission's Q' formulas.
 * mi_ul_pusch_n_srs decides n_srs from the cell's SRS configuration and the PRBs, mi_ul_pusch_resource reports what
 * the planner derives.  A MI_SRS_FLAG_LAST_SYMBOL_ONLY SRS batch run after the PUSCH batch on the same stream puts
 * the UE's own SRS into the freed symbol.  Limits: M_sc^PUSCH-initial = the current M, normal CP, FDD (no UpPTS).
 *
 * Open-loop UL power control (36.213 5.1): mi_ul_pusch_power, mi_ul_pucch_power, mi_ul_srs_power, host only, at the
 * end of this header.  Limit: no TPC accumulation (f(i) = g(i) = 0).
 *
 * srsUE's calls (phch_worker.cc) and the per-TTI calls of srslte/srslte.h over this header:
 *   srslte_ue_ul_srs_encode(&ue_ul, tti, signal)            :641 -> mi_ue_ul_srs_encode    (mi_srs_resource, srs.hip)
 *   srslte_ue_ul_srs_power(&ue_ul, PL)                      :652 -> mi_ue_ul_srs_power     (mi_ul_srs_power)
 *   srslte_ue_ul_pusch_power(&ue_ul, PL, p0_preamble)       :568 -> mi_ue_ul_pusch_power   (mi_ul_pusch_power)
 *   srslte_ue_ul_pucch_power(&ue_ul, PL, format, n_cqi, n_harq) :622 -> mi_ue_ul_pucch_power (mi_ul_pucch_power)
 * srsUE's own flow never sends the SRS together with PUCCH in one subframe; with mi_ue_ul_set_pusch_srs the PUSCH
 * encode call shortens the PUSCH in SRS subframes and lays the UE's own SRS into the freed symbol.
 */
#ifndef MI_UL_H
#define MI_UL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t cell_id, nof_prb, sf_idx, rnti;
  uint32_t n_prb, L_prb, tbs, Qm, rv;                 /* allocation (no hopping), TB bits, 2/4/6, rv 0..3 */
  uint32_t group_hopping, sequence_hopping, delta_ss;  /* DMRS cell configuration (srslte_refsignal_dmrs_pusch_cfg_t) */
  uint32_t cyclic_shift, n_dmrs2;                      /* RRC cyclicShift, DCI format 0 cyclic-shift field (0..7) */
  uint32_t ack_len, ack, I_offset_ack;                 /* HARQ-ACK on PUSCH (36.212 5.2.2.6): 0, 1 or 2 bits
                                                          (bit 0 = first), beta_offset index (36.213 8.6.3-1) */
  uint32_t hop, n_prb1;                                /* hop = 1: slot 1 starts at PRB n_prb1 (frequency hopping,
                                                          36.213 8.4 -- the per-TTI API computes it from the DCI) */
  uint32_t cqi_len, I_offset_cqi;                      /* CQI on PUSCH (36.212 5.2.2.6.4): 0..64 bits, beta_offset
                                                          index 2..15 (36.213 Table 8.6.3-3) */
  uint8_t  cqi[64];                                    /* CQI bits o_0 .. o_{O-1}, one per byte (srslte_uci_data_t) */
  uint32_t ri_len, ri, I_offset_ri;                    /* RI on PUSCH: 0..2 bits (bit 0 = o0), index 0..12 (8.6.3-2) */
  uint32_t n_srs;                                      /* 1: the last SC-FDMA symbol carries no PUSCH (a cell-specific
                                                          SRS subframe, 36.211 5.3.4): 11 data symbols, symbol 13
                                                          written as zeros.  mi_ul_pusch_n_srs decides it */
  uint32_t n_symb_initial;                             /* N_symb^PUSCH-initial of the TB's first transmission in the
                                                          Q' formulas (36.212 5.2.2.6): 11, 12, or 0 = 12 - n_srs */
} mi_ul_cfg_t;

/* what the planner derives for one transmission (36.212 5.2.2.6-5.2.2.8), and what the CPU tests compare */
typedef struct {
  uint32_t n_symb;                      /* data symbols of the subframe, 12 - n_srs */
  uint32_t G;                           /* UL-SCH coded bits: (n_symb M - Q'_CQI - Q'_RI) Qm */
  uint32_t q_ack, q_ri, q_cqi;          /* Q'_ACK, Q'_RI, Q'_CQI coded symbols */
  uint32_t C;                           /* code blocks */
  uint32_t E[16];                       /* rate-matching output bits of code blocks 0 .. C - 1 (5.1.4.1.2) */
} mi_ul_res_t;
/* host only (no device needed).  Every field of *c is checked first: 0, or -1 + mi_last_error with *r untouched.
 * mi_ul_batch_create plans through the same code.  Rejected (the error text begins "PUSCH"): n_srs > 1,
 * n_symb_initial outside {0, 11, 12}, UCI that leaves no cell for the data */
int mi_ul_pusch_resource(const mi_ul_cfg_t *c, mi_ul_res_t *r);

/* Is the PUSCH of this subframe shortened by one symbol (36.211 5.3.4)?  The cell's srs-SubframeConfig (0..14) and
 * srs-BandwidthConfig (0..7), the subframe, the first PRB of the allocation in slots 0 / 1 and its length,
 * ue_sends_srs = this UE sends its own SRS in the subframe.  Returns 0, 1, or -1 for bad arguments.
 *   MI_PUSCH_SRS_OVERLAP  1 if ue_sends_srs, or if the subframe is cell-specific SRS and the PRBs of either slot meet
 *                         the cell's sounding band [floor(N_RB / 2) - m_SRS,0 / 2, ... + m_SRS,0) (5.5.3.2)
 *   MI_PUSCH_SRS_ALL_CS   1 in every cell-specific SRS subframe and if ue_sends_srs (srsLTE's rule, for eNBs built on it)
 *   MI_PUSCH_SRS_OFF      always 0 */
enum { MI_PUSCH_SRS_OFF = 0, MI_PUSCH_SRS_OVERLAP, MI_PUSCH_SRS_ALL_CS };
int mi_ul_pusch_n_srs(uint32_t nof_prb, uint32_t srs_subframe_config, uint32_t srs_bw_cfg, uint32_t sf_idx,
                      uint32_t n_prb0, uint32_t n_prb1, uint32_t L_prb, int ue_sends_srs, uint32_t rule);

enum { MI_UL_STAGE_CRC = 0, MI_UL_STAGE_ENCODE, MI_UL_STAGE_MOD, MI_UL_NSTAGES };
#define MI_UL_FLAG_PROFILE 1u

typedef struct mi_ul_batch mi_ul_batch_t;

mi_ul_batch_t *mi_ul_batch_create(const mi_ul_cfg_t *cfgs, uint32_t n, uint32_t flags);
void   mi_ul_batch_destroy(mi_ul_batch_t *b);
/* payload layout: TB i (tbs/8 bytes, MSB first) at byte offset mi_ul_batch_payload_offset(b, i) */
size_t mi_ul_batch_payload_offset(const mi_ul_batch_t *b, uint32_t i);
size_t mi_ul_batch_payload_bytes(const mi_ul_batch_t *b);
/* output layout: subframe i (15 N cf32 samples) at cf32 offset mi_ul_batch_iq_offset(b, i) */
size_t mi_ul_batch_iq_offset(const mi_ul_batch_t *b, uint32_t i);
size_t mi_ul_batch_iq_samples(const mi_ul_batch_t *b);
uint32_t mi_ul_batch_n_codeblocks(const mi_ul_batch_t *b);
/* enqueue the chain on `stream` (hipStream_t, NULL = default): d_payload -> d_iq (both device) */
int    mi_ul_batch_run(mi_ul_batch_t *b, const void *d_payload, void *d_iq, void *stream);
/* parity hooks: the coded symbols of transmission i after the last run in channel-interleaver input order
 * (36.212 5.2.2.7 g: Q'_CQI CQI symbols, then the rate-matched data), Qm bits per byte, first bit = MSB;
 * n_symb M bytes are written (n_symb = 12 - n_srs), of which the last Q'_RI (the RI cells) are zero */
int    mi_ul_batch_symbols(mi_ul_batch_t *b, uint32_t i, uint8_t *host);
int    mi_ul_batch_stage_ms(mi_ul_batch_t *b, float *ms /* MI_UL_NSTAGES */, uint32_t *nruns);
void   mi_ul_batch_profile_reset(mi_ul_batch_t *b);
/* algorithmic HBM bytes per run: payload read + IQ write (SURVEY.md 8d convention) */
double mi_ul_batch_algo_bytes(const mi_ul_batch_t *b);

/* PUSCH frequency hopping type 2 (subband hopping, 36.211 5.3.4; selected by the DCI format 0 / RAR hopping
 * bits, 36.213 8.4 Table 8.4-1): the first PRB of the allocation n_vrb .. n_vrb + L - 1 in slot ns (0..19) of
 * the frame, given the cell's pusch-HoppingOffset n_ho, hopping subbands n_sb (>= 1), the hopping mode
 * (intra = intra- and inter-subframe, else inter-subframe) and CURRENT_TX_NB.  Every VRB is mapped by
 *   n~_PRB = (n~_VRB + f_hop(i) N_sb^RB + ((N_sb^RB - 1) - 2 (n~_VRB mod N_sb^RB)) f_m(i)) mod (N_sb^RB N_sb),
 * n~_VRB = n_VRB - N~_HO / 2 and n_PRB = n~_PRB + N~_HO / 2 (N_sb > 1; N~_HO = n_ho rounded up to even,
 * N_sb^RB = floor((N_RB - N~_HO - N_RB mod 2) / N_sb)), N_sb^RB = N_RB and no offset for N_sb = 1; f_hop and
 * f_m from the Gold sequence c(k) with c_init = N_ID^cell restarted each frame, i = ns (intra) or ns / 2.
 * Returns the lowest PRB of the mapped set, or -1 if the set is not L contiguous PRBs inside the band. */
int mi_ul_hop_type2(uint32_t nof_prb, uint32_t n_ho, uint32_t n_sb, int intra, uint32_t cell_id, uint32_t n_vrb,
                    uint32_t L, uint32_t ns, uint32_t current_tx_nb);

/* ---- PUCCH formats 1/1a/1b and 2/2a/2b (36.211 5.4, 5.5.2.2; normal CP, FDD) ------------------------- */
enum { MI_PUCCH_1 = 0, MI_PUCCH_1A, MI_PUCCH_1B, MI_PUCCH_2, MI_PUCCH_2A, MI_PUCCH_2B };
typedef struct {
  uint32_t cell_id, nof_prb, sf_idx, rnti;
  uint32_t format;                      /* MI_PUCCH_* */
  uint32_t n_pucch;                     /* n_pucch^(1) for 1/1a/1b, n_pucch^(2) for 2/2a/2b */
  uint32_t delta_shift, N_cs, n_rb_2;   /* deltaPUCCH-Shift 1..3, nCS-AN 0..7, nRB-CQI */
  uint32_t group_hopping;               /* sequence-group hopping on/off (v = 0 always: M_sc = 12) */
  uint32_t shortened;                   /* formats 1/1a/1b: last symbol of slot 1 not sent */
  uint32_t cqi_len;                     /* formats 2/2a/2b: A = 1..11 */
} mi_pucch_cfg_t;
typedef struct {                        /* everything the kernel needs, and what the CPU tests compare */
  uint32_t n_prb[2];                    /* PRB of slots 0 / 1 */
  uint32_t u[2];                        /* base-sequence group per slot */
  uint32_t n_prime[2], n_oc[2];         /* n'(ns); orthogonal-cover index (formats 1x, 0 for 2x) */
  uint32_t n_cs[2][7];                  /* cyclic shift per (slot, symbol): alpha = 2 pi n_cs / 12 */
} mi_pucch_res_t;
/* host only (no device needed).  Every field of *c is checked first: 0, or -1 + mi_last_error with *r untouched */
int mi_pucch_resource(const mi_pucch_cfg_t *c, mi_pucch_res_t *r);
/* the same for n configurations: r[i] from c[i], stopping at the first one rejected; returns how many were planned */
uint32_t mi_pucch_resource_n(const mi_pucch_cfg_t *c, uint32_t n, mi_pucch_res_t *r);
/* 36.213 10.1 (FDD): which format on which resource for this UCI.  ack_len 0..2 HARQ-ACK bits, sr = positive
 * scheduling request, cqi_len = CQI bits to report (simul_cqi_ack_dropped = 1: simultaneousAckNackAndCQI is off,
 * a CQI that meets a HARQ-ACK is dropped and the HARQ-ACK goes alone).  A CQI that meets a positive SR is
 * dropped.  Returns the format and writes the resource to *n_pucch; -1 = nothing to send. */
int mi_pucch_select(uint32_t ack_len, int sr, uint32_t cqi_len, int simul_cqi_ack_dropped, uint32_t n_cce,
                    uint32_t N_pucch_1, uint32_t n_pucch_2, uint32_t n_pucch_sr, uint32_t *n_pucch);

/* UCI word of one transmission: bits 0-1 HARQ-ACK (bit 0 = first), bits 8-18 CQI bits o_0 .. o_10 */
#define MI_PUCCH_UCI(ack, cqi) (((uint32_t)(ack) & 3u) | (((uint32_t)(cqi) & 0x7FFu) << 8))
typedef struct mi_pucch_batch mi_pucch_batch_t;
mi_pucch_batch_t *mi_pucch_batch_create(const mi_pucch_cfg_t *cfgs, uint32_t n, uint32_t flags);
void   mi_pucch_batch_destroy(mi_pucch_batch_t *b);
/* output layout: subframe i (15 N cf32 samples) at cf32 offset mi_pucch_batch_iq_offset(b, i) */
size_t mi_pucch_batch_iq_offset(const mi_pucch_batch_t *b, uint32_t i);
size_t mi_pucch_batch_iq_samples(const mi_pucch_batch_t *b);
/* enqueue on `stream` (hipStream_t, NULL = default): d_uci (n device uint32 words) -> d_iq; the plan is reused
 * across runs, every sample of every subframe is written */
int    mi_pucch_batch_run(mi_pucch_batch_t *b, const uint32_t *d_uci, void *d_iq, void *stream);
/* parity hook: the planned resource of transmission i */
int    mi_pucch_batch_resource(const mi_pucch_batch_t *b, uint32_t i, mi_pucch_res_t *r);

/* ---- PRACH preamble, formats 0-3 (36.211 5.7; FDD, N_ZC = 839) --------------------------------------- */
typedef struct {
  uint32_t nof_prb;          /* 6, 15, 25, 50, 75, 100 */
  uint32_t config_idx;       /* prach-ConfigIndex 0..63 (30, 46, 60, 61, 62 are N/A) */
  uint32_t root_seq_idx;     /* rootSequenceIndex (logical) 0..837 */
  uint32_t zero_corr_zone;   /* zeroCorrelationZoneConfig 0..15 (0..14 when high_speed) */
  uint32_t high_speed;       /* restricted set */
  uint32_t freq_offset;      /* n_PRBoffset^RA, 0..nof_prb-6 */
  uint32_t preamble_idx;     /* 0..63 */
} mi_prach_cfg_t;
typedef struct {                        /* everything the kernels need, and what the CPU tests compare */
  uint32_t format, N_ifft, N_cp, N_seq, N_cs;   /* N_ifft = 12 srslte_symbol_sz(nof_prb); samples at the UL rate */
  uint32_t u, C_v;                      /* physical root and cyclic shift of preamble_idx */
  uint32_t first_bin;                   /* bin of X(0) in the N_ifft-point grid: (13 + 12 k0) mod N_ifft */
  uint32_t n_roots;                     /* distinct roots the cell's 64 preambles use */
} mi_prach_res_t;
/* host only (no device needed).  Every field of *c is checked first: 0, or -1 + mi_last_error with *r untouched.  A
 * restricted-set configuration whose 838 roots give fewer than 64 preambles is rejected. */
int mi_prach_resource(const mi_prach_cfg_t *c, mi_prach_res_t *r);
/* the same for n configurations: r[i] from c[i], stopping at the first one rejected; returns how many were planned */
uint32_t mi_prach_resource_n(const mi_prach_cfg_t *c, uint32_t n, mi_prach_res_t *r);
/* Table 5.7.2-4: the physical root u of a logical index, -1 if it is > 837 */
int mi_prach_root(uint32_t logical_idx);
/* Table 5.7.1-2 (FDD): the preamble format 0..3 of a prach-ConfigIndex, -1 for the N/A rows and indices > 63 */
int mi_prach_format(uint32_t config_idx);
/* 1 iff a preamble may start in subframe tti % 10 of frame tti / 10 under config_idx and allowed_subframe is -1 or
 * that subframe (srsUE prach.cc:130); 0 for the N/A rows */
int mi_prach_send_tti(uint32_t config_idx, uint32_t tti, int allowed_subframe);

/* a workgroup owns one residue of the polyphase transform instead of up to 4 adjacent ones (A/B: DESIGN.md) */
#define MI_PRACH_FLAG_SINGLE_RESIDUE 1u
typedef struct mi_prach_batch mi_prach_batch_t;
mi_prach_batch_t *mi_prach_batch_create(const mi_prach_cfg_t *cfgs, uint32_t n, uint32_t flags);
void   mi_prach_batch_destroy(mi_prach_batch_t *b);
/* output layout: transmission i (N_cp + N_seq cf32 samples, CP first) at cf32 offset mi_prach_batch_iq_offset(b, i) */
size_t mi_prach_batch_iq_offset(const mi_prach_batch_t *b, uint32_t i);
size_t mi_prach_batch_iq_samples(const mi_prach_batch_t *b);
/* enqueue on `stream` (hipStream_t, NULL = default).  d_cfo: n device floats, the frequency shift of each
 * transmission in subcarriers of 15 kHz (sample i, counted from the first CP sample, is multiplied by
 * exp(j 2 pi cfo i / N_ul)), NULL = none; d_scale: n device floats, NULL = 1.  Normalisation: unit power per PRACH
 * subcarrier (mean power 839 / N_ifft over the sequence).  The plan is reused across runs (one run of a batch at a
 * time), every sample of every transmission is written */
int    mi_prach_batch_run(mi_prach_batch_t *b, const float *d_cfo, const float *d_scale, void *d_iq, void *stream);
/* parity hook: the planned resource of transmission i */
int    mi_prach_batch_resource(const mi_prach_batch_t *b, uint32_t i, mi_prach_res_t *r);

/* ---- SRS, periodic (36.211 5.5.3, 36.213 8.2; FDD, normal CP, one antenna port) ------------------------ */
typedef struct {
  uint32_t cell_id, nof_prb, tti;       /* tti 0..10239: subframe tti % 10 of frame tti / 10 */
  uint32_t bw_cfg;                      /* cell: srs-BandwidthConfig C_SRS 0..7 */
  uint32_t B, b_hop, n_rrc, k_tc;       /* UE: srs-Bandwidth 0..3, srs-HoppingBandwidth 0..3, freqDomainPosition
                                           0..23, transmissionComb 0/1 */
  uint32_t n_srs, I_srs;                /* UE: cyclicShift 0..7, srs-ConfigIndex 0..636 (637.. reserved) */
  uint32_t group_hopping, sequence_hopping, delta_ss;   /* the cell's UL reference-signal configuration */
} mi_srs_cfg_t;
typedef struct {                        /* everything the kernel needs, and what the CPU tests compare */
  uint32_t m_srs, M_sc;                 /* m_SRS,B in PRBs, sequence length 6 m_srs */
  uint32_t k0;                          /* first subcarrier, 0 .. 12 nof_prb - 1; the SRS occupies k0 + 2 k' */
  uint32_t n_b[4];                      /* frequency position index per level b <= B (0 above B) */
  uint32_t n_SRS, T_srs;                /* transmission counter floor(tti / T_SRS), periodicity in subframes */
  uint32_t u, v;                        /* sequence group and base sequence number in slot 2 (tti % 10) + 1 */
  uint32_t nzc, q;                      /* Zadoff-Chu length and root; nzc = 0: the tabulated M_sc = 24 sequence of
                                           group q = u */
  uint32_t n_cs;                        /* alpha = 2 pi n_cs / 8 */
} mi_srs_res_t;
/* host only (no device needed).  Every field of *c is checked first: 0, or -1 + mi_last_error with *r untouched.  A
 * configuration whose m_SRS,0 exceeds nof_prb is rejected (6 PRB admits only C_SRS = 7). */
int mi_srs_resource(const mi_srs_cfg_t *c, mi_srs_res_t *r);
/* the same for n configurations: r[i] from c[i], stopping at the first one rejected; returns how many were planned */
uint32_t mi_srs_resource_n(const mi_srs_cfg_t *c, uint32_t n, mi_srs_res_t *r);

/* write only the N + CP samples of symbol 13 of every subframe and leave the rest as it was: the SRS laid over a
 * shortened PUCCH subframe that mi_pucch_batch_run wrote before it on the same stream */
#define MI_SRS_FLAG_LAST_SYMBOL_ONLY 1u
typedef struct mi_srs_batch mi_srs_batch_t;
mi_srs_batch_t *mi_srs_batch_create(const mi_srs_cfg_t *cfgs, uint32_t n, uint32_t flags);
void   mi_srs_batch_destroy(mi_srs_batch_t *b);
/* output layout: subframe i (15 N cf32 samples) at cf32 offset mi_srs_batch_iq_offset(b, i) */
size_t mi_srs_batch_iq_offset(const mi_srs_batch_t *b, uint32_t i);
size_t mi_srs_batch_iq_samples(const mi_srs_batch_t *b);
/* enqueue on `stream` (hipStream_t, NULL = default).  d_cfo: n device floats, the frequency shift of each
 * transmission in subcarriers (sample i of the subframe is multiplied by exp(j 2 pi cfo i / N)), NULL = none;
 * d_scale: n device floats, NULL = 1.  Normalisation: unit power per occupied subcarrier.  The plan is reused across
 * runs; every sample of every subframe is written (symbols 0..12 with zeros) unless MI_SRS_FLAG_LAST_SYMBOL_ONLY */
int    mi_srs_batch_run(mi_srs_batch_t *b, const float *d_cfo, const float *d_scale, void *d_iq, void *stream);
/* parity hook: the planned resource of transmission i */
int    mi_srs_batch_resource(const mi_srs_batch_t *b, uint32_t i, mi_srs_res_t *r);

/* ---- open-loop UL power control (36.213 5.1.1.1, 5.1.2.1, 5.1.3.1), host only --------------------------- */
typedef struct {                        /* the fields of srslte_ue_ul_powerctrl_t, dB / dBm */
  float p0_nominal_pusch, alpha, p0_nominal_pucch;
  float delta_f_pucch[5];               /* deltaF-PUCCH of formats 1, 1b, 2, 2a, 2b (1a is the reference: 0) */
  float delta_preamble_msg3, p0_ue_pusch;
  uint32_t delta_mcs_based;             /* deltaMCS-Enabled: K_S = 1.25, else 0 */
  uint32_t acc_enabled;                 /* stored, unused: the TPC accumulations f(i) = g(i) = 0 */
  float p0_ue_pucch, p_srs_offset;      /* p_srs_offset: the RRC value pSRS-Offset 0..15 */
} mi_ul_power_cfg_t;
#define MI_UL_P_CMAX 23.0f              /* dBm, power class 3; every result is capped at it */
/* P_PUSCH = 10 log10(L_prb) + P0 + alpha PL + Delta_TF.  P0 = p0_nominal_pusch + p0_ue_pusch; for a grant of the
 * random-access response (p0_preamble != 0) P0 = p0_preamble + delta_preamble_msg3 and alpha = 1.  Delta_TF =
 * 10 log10(2^(1.25 BPRE) - 1), BPRE = sum_Kr / (144 L_prb) (sum_Kr: the code-block sizes of the TB in bits; 12
 * data symbols), when delta_mcs_based, else 0 */
float mi_ul_pusch_power(const mi_ul_power_cfg_t *p, float PL, float p0_preamble, uint32_t L_prb, uint32_t sum_Kr);
/* the same with N_RE = 12 L_prb n_symb_initial (11 when the TB's first transmission was shortened for the SRS);
 * mi_ul_pusch_power is this at n_symb_initial = 12.  0 for n_symb_initial = 0 */
float mi_ul_pusch_power_nsymb(const mi_ul_power_cfg_t *p, float PL, float p0_preamble, uint32_t L_prb, uint32_t sum_Kr,
                              uint32_t n_symb_initial);
/* P_PUCCH = p0_nominal_pucch + p0_ue_pucch + PL + h(n_cqi, n_harq) + Delta_F(format).  format: MI_PUCCH_*; h =
 * 10 log10(n_cqi / 4) for formats 2/2a/2b with n_cqi >= 4, else 0 (normal CP) */
float mi_ul_pucch_power(const mi_ul_power_cfg_t *p, float PL, uint32_t format, uint32_t n_cqi, uint32_t n_harq);
/* P_SRS = P_SRS_OFFSET + 10 log10(m_srs) + P0_PUSCH + alpha PL.  P_SRS_OFFSET = -3 + p_srs_offset when
 * delta_mcs_based (K_S = 1.25), else -10.5 + 1.5 p_srs_offset */
float mi_ul_srs_power(const mi_ul_power_cfg_t *p, float PL, uint32_t m_srs);

#ifdef __cplusplus
}
#endif
#endif
