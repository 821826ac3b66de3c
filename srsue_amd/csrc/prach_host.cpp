// prach_host.cpp -- host planner of the PRACH preamble transmitter (see prach.h; no HIP calls).  Spec arithmetic:
// 36.211 5.7.1 (formats, Table 5.7.1-2 timing, FDD), 5.7.2 (logical roots, N_CS, cyclic shifts of the unrestricted
// and restricted sets, preamble numbering), 5.7.3 (frequency mapping).  DESIGN.md carries the formulas as implemented.
#include "prach.h"

#include <algorithm>

#include "plan.h"   // set_error

namespace mi {
namespace {

constexpr uint32_t NZC = PRACH_NZC;

// Table 5.7.2-4, formats 0-3: the first root of every pair in logical order; logical 2 i is ROOT_PAIR[i], logical
// 2 i + 1 its complement 839 - ROOT_PAIR[i].  The order of the pairs inside a group is a transcription that the
// group properties (tests/test_prach_ref.py) cannot check: DESIGN.md.
const uint16_t ROOT_PAIR[419] = {
    129, 140, 120, 210, 168, 84, 105, 93, 70, 60, 2, 1,                                                // 0-23
    56, 112, 148,                                                                                      // 24-29
    80, 42, 40,                                                                                        // 30-35
    35, 73, 146,                                                                                       // 36-41
    31, 28, 30, 27, 29,                                                                                // 42-51
    24, 48, 68, 74, 178, 136,                                                                          // 52-63
    86, 78, 43, 39, 20, 21,                                                                            // 64-75
    95, 202, 190, 181, 137, 125, 151,                                                                  // 76-89
    217, 128, 142, 122, 203, 118, 110, 89, 103, 61, 55, 15, 14,                                        // 90-115
    12, 23, 34, 37, 46, 207, 179, 145, 130, 223,                                                       // 116-135
    228, 227, 132, 133, 143, 135, 161, 201, 173, 106, 83, 91, 66, 53, 10, 9,                           // 136-167
    7, 8, 16, 47, 64, 57, 104, 101, 108, 208, 184, 197, 191, 121, 141, 149, 216, 218,                  // 168-203
    152, 144, 134, 138, 199, 162, 176, 119, 158, 164, 174, 171, 170, 87, 169, 88, 107, 81, 82, 100,
    98, 71, 59, 65, 50, 49, 26, 17, 13, 6,                                                             // 204-263
    5, 33, 51, 75, 99, 96, 97, 166, 172, 175, 187, 163, 185, 200, 114, 189, 115, 194, 195, 192, 182,
    157, 156, 211, 154, 123, 139, 212, 153, 213, 215, 150,                                             // 264-327
    225, 224, 221, 220, 127, 147, 124, 193, 205, 206, 116, 160, 186, 167, 79, 85, 77, 92, 58, 62, 69,
    54, 36, 32, 25, 18, 11, 4,                                                                         // 328-383
    3, 19, 22, 41, 38, 44, 52, 45, 63, 67, 72, 76, 94, 102, 90, 109, 165, 111, 209, 204, 117, 188, 159,
    198, 113, 183, 180, 177, 196, 155, 214, 126, 131, 219, 222, 226,                                   // 384-455
    230, 232, 262, 252, 418, 416, 413, 411, 376, 395, 283, 285, 379, 390, 363, 384, 388, 386, 361, 387,
    360, 310, 354, 328, 315, 337, 349, 335, 324,                                                       // 456-513
    323, 320, 334, 359, 295, 385, 292, 291, 381, 399, 380, 397, 369, 377, 410, 407, 281, 414, 247, 277,
    271, 272, 264, 259,                                                                                // 514-561
    237, 239, 244, 243, 275, 278, 250, 246, 417, 248, 394, 393, 370, 365, 300, 299, 364, 362, 298, 312,
    313, 314, 353, 352, 343, 327, 350, 326, 319, 332, 333, 348, 347, 322,                              // 562-629
    330, 338, 341, 340, 342, 301, 366, 401, 371, 408, 375, 249, 269, 238, 234,                         // 630-659
    257, 273, 255, 254, 245, 251, 412, 372, 282, 403, 396, 392, 391, 382, 389, 294, 297, 311, 344, 345,
    318, 331, 325, 321,                                                                                // 660-707
    346, 339, 351, 306, 289, 400, 378, 374, 415, 270, 241,                                             // 708-729
    231, 260, 268, 276, 409, 398, 290, 304, 308, 358, 316,                                             // 730-751
    293, 288, 284, 368, 253, 256, 263,                                                                 // 752-765
    242, 274, 402, 383, 357, 329,                                                                      // 766-777
    317, 307, 286, 287, 266, 261,                                                                      // 778-789
    236, 303, 356,                                                                                     // 790-795
    355, 405, 404, 406,                                                                                // 796-803
    235, 267, 302,                                                                                     // 804-809
    309, 265, 233,                                                                                     // 810-815
    367, 296,                                                                                          // 816-819
    336, 305, 373, 280, 279, 419, 240, 258, 229};                                                      // 820-837

// Table 5.7.2-2: N_CS by zeroCorrelationZoneConfig
const uint16_t NCS_UNRESTRICTED[16] = {0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419};
const uint16_t NCS_RESTRICTED[15] = {15, 18, 22, 26, 32, 38, 46, 55, 68, 82, 100, 128, 158, 202, 237};

// Table 5.7.1-2 (FDD): the subframes of row config_idx % 16 as a bit mask, and whether only even frames carry PRACH
const uint16_t ROW_SUBFRAMES[16] = {1u << 1, 1u << 4, 1u << 7, 1u << 1, 1u << 4, 1u << 7, (1u << 1) | (1u << 6),
                                    (1u << 2) | (1u << 7), (1u << 3) | (1u << 8), (1u << 1) | (1u << 4) | (1u << 7),
                                    (1u << 2) | (1u << 5) | (1u << 8), (1u << 3) | (1u << 6) | (1u << 9),
                                    0x155, 0x2AA, 0x3FF, 1u << 9};
bool row_even_only(uint32_t row) { return row < 3 || row == 15; }

uint32_t physical_root(uint32_t logical) {
  const uint32_t a = ROOT_PAIR[logical / 2];
  return logical & 1u ? NZC - a : a;
}

// the cyclic shifts of one root in increasing v (at most max of them are written); returns how many the root has
uint32_t shifts_of_root(uint32_t u, uint32_t N_cs, bool restricted, uint32_t* C_v, uint32_t max) {
  uint32_t n = 0;
  if (!restricted) {
    const uint32_t count = N_cs ? NZC / N_cs : 1;
    for (; n < count && n < max; n++) C_v[n] = n * N_cs;
    return count;
  }
  uint32_t p = 1;
  while ((p * u) % NZC != 1) p++;   // u^-1 mod 839 (839 is prime, u = 1..838)
  const uint32_t d_u = 2 * p < NZC ? p : NZC - p;
  uint32_t n_shift, d_start, n_group, nbar;
  if (N_cs <= d_u && 3 * d_u < NZC) {
    n_shift = d_u / N_cs;
    d_start = 2 * d_u + n_shift * N_cs;
    n_group = NZC / d_start;
    const int rest = (int)NZC - 2 * (int)d_u - (int)(n_group * d_start);
    nbar = rest > 0 ? (uint32_t)rest / N_cs : 0;
  } else if (3 * d_u >= NZC && 2 * d_u + N_cs <= NZC) {
    n_shift = (NZC - 2 * d_u) / N_cs;
    d_start = NZC - 2 * d_u + n_shift * N_cs;
    n_group = d_u / d_start;
    const int rest = (int)d_u - (int)(n_group * d_start);
    nbar = std::min(rest > 0 ? (uint32_t)rest / N_cs : 0u, n_shift);
  } else {
    return 0;
  }
  const uint32_t count = n_shift * n_group + nbar;
  for (; n < count && n < max; n++) C_v[n] = d_start * (n / n_shift) + (n % n_shift) * N_cs;
  return count;
}

int format_of(uint32_t config_idx) {
  // row 14 exists for format 0 only (30, 46, 62 are N/A), and so are rows 12 and 13 of format 3 (60, 61)
  if (config_idx > 63 || config_idx == 30 || config_idx == 46 || (config_idx >= 60 && config_idx <= 62)) return -1;
  return (int)(config_idx / 16);
}

// srsUE configures one cell at a time: its 64 preambles are derived once per thread and configuration
struct CellMemo {
  uint32_t root = 0xFFFFFFFFu, zczc = 0, hs = 0;
  PrachCell cell;
};
thread_local CellMemo g_cell;

// every field of c; the cell's preambles to *cell.  false + set_error
bool check(const mi_prach_cfg_t& c, const PrachCell** cell) {
  if (!std_nof_prb(c.nof_prb)) {
    set_error("PRACH: nof_prb must be one of 6, 15, 25, 50, 75, 100");
    return false;
  }
  if (format_of(c.config_idx) < 0) {
    set_error("PRACH: prach-ConfigIndex must be 0..63 and not 30, 46, 60, 61, 62 (formats 0-3, FDD)");
    return false;
  }
  if (c.freq_offset > c.nof_prb - 6) {
    set_error("PRACH: prach-FreqOffset must leave 6 PRBs inside the cell (freq_offset <= nof_prb - 6)");
    return false;
  }
  if (c.preamble_idx > 63) {
    set_error("PRACH: preamble index must be 0..63");
    return false;
  }
  const uint32_t hs = c.high_speed ? 1u : 0u;
  if (g_cell.root != c.root_seq_idx || g_cell.zczc != c.zero_corr_zone || g_cell.hs != hs) {
    g_cell.root = 0xFFFFFFFFu;
    if (!prach_cell(c.root_seq_idx, c.zero_corr_zone, hs, &g_cell.cell)) return false;
    g_cell.root = c.root_seq_idx;
    g_cell.zczc = c.zero_corr_zone;
    g_cell.hs = hs;
  }
  *cell = &g_cell.cell;
  return true;
}

void derive(const mi_prach_cfg_t& c, const PrachCell& cell, mi_prach_res_t* r) {
  static const uint32_t CP[4] = {3168, 21024, 6240, 21024}, REP[4] = {1, 1, 2, 2};
  const uint32_t N_ul = (uint32_t)symbol_sz(c.nof_prb), f = (uint32_t)format_of(c.config_idx);
  r->format = f;
  r->N_ifft = 12 * N_ul;
  r->N_cp = CP[f] * N_ul / 2048;
  r->N_seq = REP[f] * r->N_ifft;
  r->N_cs = c.high_speed ? NCS_RESTRICTED[c.zero_corr_zone] : NCS_UNRESTRICTED[c.zero_corr_zone];
  r->u = cell.u[c.preamble_idx];
  r->C_v = cell.C_v[c.preamble_idx];
  // 5.7.3: phi + K (k0 + 1 / 2) = 13 + 12 k0 with k0 = 12 n_PRBoffset - 6 N_RB (phi = 7, K = 12)
  const int k0 = 12 * (int)c.freq_offset - 6 * (int)c.nof_prb;
  const int fb = (13 + 12 * k0) % (int)r->N_ifft;
  r->first_bin = (uint32_t)(fb < 0 ? fb + (int)r->N_ifft : fb);
  r->n_roots = cell.n_roots;
}

}  // namespace

bool prach_cell(uint32_t root_seq_idx, uint32_t zero_corr_zone, uint32_t high_speed, PrachCell* out) {
  if (root_seq_idx > 837) {
    set_error("PRACH: rootSequenceIndex must be 0..837");
    return false;
  }
  if (zero_corr_zone > (high_speed ? 14u : 15u)) {
    set_error("PRACH: zeroCorrelationZoneConfig must be 0..15 (0..14 for the restricted set)");
    return false;
  }
  const uint32_t N_cs = high_speed ? NCS_RESTRICTED[zero_corr_zone] : NCS_UNRESTRICTED[zero_corr_zone];
  uint32_t n = 0, roots = 0;
  for (uint32_t i = 0; i < 838 && n < 64; i++) {
    const uint32_t u = physical_root((root_seq_idx + i) % 838);
    const uint32_t got = std::min(shifts_of_root(u, N_cs, high_speed != 0, out->C_v + n, 64 - n), 64 - n);
    for (uint32_t k = 0; k < got; k++) out->u[n + k] = u;
    n += got;
    roots += got ? 1 : 0;
  }
  if (n < 64) {
    set_error("PRACH: the 838 roots give fewer than 64 preambles for this restricted-set configuration");
    return false;
  }
  out->n_roots = roots;
  return true;
}

int PrachPlan::build(const mi_prach_cfg_t* cfgs, uint32_t n) {
  txs.clear();
  res.clear();
  roots.clear();
  items.clear();
  iq_samples = 0;
  std::vector<mi_prach_res_t> rs(n);
  for (uint32_t i = 0; i < n; i++) {   // every configuration is checked before anything is kept
    const PrachCell* cell;
    if (!check(cfgs[i], &cell)) return -1;
    derive(cfgs[i], *cell, &rs[i]);
  }
  for (uint32_t i = 0; i < n; i++) {
    const mi_prach_res_t& r = rs[i];
    MiPrachTx t{};
    t.iq_off = iq_samples;
    t.N_ifft = r.N_ifft;
    t.N_ul = r.N_ifft / 12;
    t.L = r.N_ifft / PRACH_NFFT;
    t.N_cp = r.N_cp;
    t.reps = r.N_seq / r.N_ifft;
    t.C_v = r.C_v;
    t.first_bin = r.first_bin;
    const auto it = std::find(roots.begin(), roots.end(), r.u);   // roots are deduplicated across transmissions
    t.root_slot = (uint32_t)(it - roots.begin());
    if (it == roots.end()) roots.push_back(r.u);
    // a workgroup owns rpw adjacent residues: the largest of 4, 2, 1 that divides L, capped by the variant
    uint32_t rpw = std::min(rpw_cap, PRACH_RPW_MAX);
    while (t.L % rpw) rpw /= 2;
    for (uint32_t r0 = 0; r0 < t.L; r0 += rpw) items.push_back(MiPrachItem{i, r0, rpw});
    iq_samples += (size_t)r.N_cp + r.N_seq;
    txs.push_back(t);
  }
  res = std::move(rs);
  return 0;
}

}  // namespace mi

extern "C" {

uint32_t mi_prach_resource_n(const mi_prach_cfg_t* c, uint32_t n, mi_prach_res_t* r) {
  if (!c || !r) { mi::set_error("PRACH: null argument"); return 0; }
  for (uint32_t i = 0; i < n; i++) {
    const mi::PrachCell* cell;
    if (!mi::check(c[i], &cell)) return i;
    mi::derive(c[i], *cell, &r[i]);
  }
  return n;
}

int mi_prach_resource(const mi_prach_cfg_t* c, mi_prach_res_t* r) { return mi_prach_resource_n(c, 1, r) == 1 ? 0 : -1; }

int mi_prach_root(uint32_t logical_idx) { return logical_idx > 837 ? -1 : (int)mi::physical_root(logical_idx); }

int mi_prach_format(uint32_t config_idx) { return mi::format_of(config_idx); }

int mi_prach_send_tti(uint32_t config_idx, uint32_t tti, int allowed_subframe) {
  if (mi::format_of(config_idx) < 0) return 0;
  const uint32_t row = config_idx % 16, sf = tti % 10;
  if (mi::row_even_only(row) && ((tti / 10) & 1u)) return 0;
  if (!((mi::ROW_SUBFRAMES[row] >> sf) & 1u)) return 0;
  return allowed_subframe == -1 || allowed_subframe == (int)sf ? 1 : 0;
}

}  // extern "C"
