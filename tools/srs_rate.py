#!/usr/bin/env python3
"""SRS encode rates on the GPU (SRS): transmissions per second of mi_srs_batch_run for small and large
batches (one launch, bandwidths, hopping and cyclic shifts mixed, HIP events around the call), with and without
MI_SRS_FLAG_LAST_SYMBOL_ONLY, and microseconds per call of the per-TTI mi_ue_ul_srs_encode (host clock inside
tests/c/ue_srs_harness: plan, table upload, kernel, IQ download and copy-out) beside mi_ue_ul_pucch_encode's figure
from tests/c/ue_pucch_harness in the same run.

Warm-up, then repeated timed calls; reports the median and the spread (min .. max).  There is no earlier path to
compare with: the figures are a record."""
import argparse
import struct

import numpy as np
import torch

from pucch_rate import per_tti as per_tti_pucch
from rate_common import need_gpu, report, run_harness, stats, timed   # puts the repository root on sys.path
from srsue_amd import abi

# (bw_cfg, B) that every transmission of a bandwidth cycles through: 6 PRB admits only C_SRS 7
SHAPES = {6: [(7, 0)], 100: [(0, 0), (0, 1), (0, 2), (0, 3), (2, 0), (5, 1), (7, 0), (7, 3)]}


def batch_rate(n, nof_prb, flags, warmup, repeats):
    cfgs = []
    for i in range(n):
        bw_cfg, B = SHAPES[nof_prb][i % len(SHAPES[nof_prb])]
        cfgs.append(abi.srs_cfg(cell_id=i % 504, nof_prb=nof_prb, tti=i % 10240, bw_cfg=bw_cfg, B=B, b_hop=0, n_rrc=i % 24,
                                k_tc=i & 1, n_srs=i % 8, I_srs=i % 637, group_hopping=(i >> 1) & 1))
    b = abi.SrsBatch(cfgs, flags=flags)
    d_iq = torch.zeros(2 * b.iq_samples, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: b.run(d_iq.data_ptr(), st), warmup, repeats)
    N = 2048 if nof_prb == 100 else 128
    written = (N + 144 * N // 2048) * n if flags else b.iq_samples
    out = dict(stats(ms, n), transmissions=n, nof_prb=nof_prb, last_symbol_only=bool(flags),
               iq_gbytes_per_s=float(8 * written / (np.median(ms) * 1e6)))
    b.close()
    return out


def per_tti(nof_prb, repeats):
    """three SRS instants of a hopping configuration, each repeated `repeats` times"""
    bw_cfg, B = (7, 0) if nof_prb == 6 else (0, 1)
    ttis = [2, 12, 22]
    rec = struct.pack("20i", 1, nof_prb, len(ttis), 0, 0, 0, 0, 1, 0, bw_cfg, 9, B, 0, 5, 0, 3, 0, 0x46, 0, 0)
    rec += struct.pack("16f", *([0.0] * 16)) + struct.pack(f"{len(ttis)}i", *ttis)
    return run_harness("ue_srs_harness", rec, repeats, nof_prb=nof_prb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--tti-repeats", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = {"device": need_gpu("srs_rate.py"),
         "batch": [batch_rate(n, prb, fl, a.warmup, a.repeats) for prb in (6, 100) for fl in (0, 1) for n in a.batches],
         "per_tti": [per_tti(prb, a.tti_repeats) for prb in (6, 100)],
         "per_tti_pucch": [per_tti_pucch(prb, a.tti_repeats) for prb in (6, 100)]}
    report(r, a.out)


if __name__ == "__main__":
    main()
