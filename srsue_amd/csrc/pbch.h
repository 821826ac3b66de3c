// pbch.h -- PBCH receiver (36.211 6.6, 36.212 5.3.1): descriptors, launchers and the host engine that
// plans soft-bit extraction and the blind (ports, frames combined, 40 ms phase) decode over the grid and
// channel estimates of an Engine.
#pragma once
#include <vector>

#include "engine.h"

namespace mi {

constexpr uint32_t PBCH_RE = 240;            // REs per radio frame (normal CP)
constexpr uint32_t PBCH_BITS = 2 * PBCH_RE;  // soft bits per radio frame
constexpr uint32_t PBCH_E = 4 * PBCH_BITS;   // rate-matched bits of one BCH TTI (40 ms)
constexpr uint32_t PBCH_A = 24, PBCH_D = 40; // MIB bits, with CRC16

struct MiPbchFrame {         // one per PBCH frame (a subframe 0 of the batch)
  uint64_t grid_off, ce_off; // float2 offsets (port p of ce at ce_off + p * plane)
  uint32_t plane;            // 14 * 12 N_RB
  uint32_t ports;            // CRS ports of the subframe's cfg: the 2-port hypothesis exists iff 2
  uint32_t re_off;           // cdata offset: re[240] (grid indices)
  uint32_t pad;
};

struct MiPbchJob {           // one (candidate, port hypothesis, depth f, phase) of the blind decode
  uint32_t llr_off[4];       // float offsets of the f frames' soft bits (this hypothesis), oldest first
  uint32_t f, phase0;        // frame i sits at 40 ms phase phase0 + i (phase0 + f - 1 <= 3)
  uint32_t scr_off;          // cdata offset: 60 words = 1920 scrambling bits of the cell
  uint32_t mask;             // CRC mask of the hypothesis (36.212 Table 5.3.1.1-1)
};
struct MiPbchRes { uint32_t found; uint32_t bits; };   // bits: the 24 MIB bits, first bit = bit 23

void launch_pbch_llr(const float2* grid, const float2* ce, const MiPbchFrame* frames, const uint32_t* cdata, float* llr,
                     uint32_t n_frames, float noise, hipStream_t st);
void launch_pbch_decode(const float* llr, const MiPbchJob* jobs, const uint32_t* cdata, uint32_t rank_off,
                        MiPbchRes* res, uint32_t n_jobs, hipStream_t st);

// the 240 PBCH REs of a cell in mapping order (grid index l * 12 N_RB + k); host only
void pbch_re_list(uint32_t cell_id, uint32_t nof_prb, uint32_t* re240);

struct PbchFound { uint32_t found, nof_ports, sfn_offset, n_frames_used; uint8_t bits[PBCH_A]; };

struct PbchEngine {
  // the frames: built once from a plan (its subframes with sf_idx 0, in batch order)
  std::vector<MiPbchFrame> frames;
  std::vector<int32_t> frame_of_sf;       // batch subframe -> frame index, -1 = not a subframe 0
  std::vector<uint32_t> frame_cell;       // per frame: the plan's cell index
  std::vector<uint32_t> frame_scr;        // per frame: cdata offset of the cell's scrambling words
  std::vector<uint32_t> cdata;
  uint32_t rank_off = 0;
  // the candidates and their jobs (set_candidates)
  std::vector<MiPbchJob> jobs;
  std::vector<uint8_t> job_ports, job_f, job_phase;
  std::vector<uint32_t> job_begin;        // per candidate: jobs [job_begin[c], job_begin[c+1]) in search order
  DevBuf d_frames, d_cdata, d_jobs, d_llr, d_res;
  std::vector<MiPbchRes> res;
  size_t llr_floats() const { return frames.size() * 2 * PBCH_BITS; }
  int build(const Plan& P);
  int upload(hipStream_t st);
  // candidate c = n_frames[c] (1..4) batch subframes sf[4 c ..], oldest first; every one a subframe 0 of the
  // same cell.  Rejected (-1, set_error) before anything reaches the device
  int set_candidates(const Plan& P, const uint32_t* sf, const uint32_t* n_frames, uint32_t n_cand, hipStream_t st);
  // stages: 1 = soft bits, 2 = decode
  int run(const float2* grid, const float2* ce, uint32_t mask, float noise, hipStream_t st);
  int download(hipStream_t st);
  PbchFound select(uint32_t cand) const;
};

}  // namespace mi
