// cqi_table.h -- the SNR (dB) -> CQI index threshold table of srslte_cqi_from_snr, one copy for the host getter
// (srslte_util.cpp) and the CSI kernel's tail (csi_body.h).
#pragma once
#include "dl_common.h"

namespace mi {

// CQI c + 1 is the highest whose threshold the SNR reaches; below the first threshold (or not a number) CQI 0
__host__ __device__ inline uint8_t cqi_from_snr_db(float snr) {
  const float thr[15] = {1.95f, 4.0f, 6.0f, 8.0f, 10.0f, 11.95f, 14.05f, 16.0f,
                         17.9f, 19.9f, 21.5f, 23.45f, 25.0f, 27.3f, 29.0f};
#pragma unroll
  for (int c = 14; c >= 0; c--)
    if (snr >= thr[c]) return (uint8_t)(c + 1);
  return 0;
}

}  // namespace mi
