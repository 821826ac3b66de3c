#!/usr/bin/env python3
"""PRACH preamble rates on the GPU (PRACH): preambles per second of mi_prach_batch_run for the 64
preambles of a cell at 6 and 100 PRB, formats 0 and 3 (one run = prach_root_kernel + prach_gen_kernel, HIP events
around the call), with a workgroup owning up to 4 adjacent residues (the default) and one residue
(MI_PRACH_FLAG_SINGLE_RESIDUE); the IQ write rate of each run next to that of a plain fill of the same buffer
timed the same way; and, under the host clock inside tests/c/ue_prach_harness, microseconds per call of
mi_prach_gen (preambles already on the device: one copy) and mi_prach_gen_cfo (plan, upload, two kernels, copy),
and the wall time of init + 64 x gen on a fresh instance.

Warm-up, then repeated timed calls; reports the median and the spread (min .. max).  There is no earlier path to
compare with: the figures are a record."""
import argparse
import struct

import numpy as np
import torch

from rate_common import need_gpu, report, run_harness, timed   # puts the repository root on sys.path
from srsue_amd import abi

CELL = dict(root_seq_idx=22, zero_corr_zone=12, high_speed=0)   # N_CS = 119: 7 shifts per root, 10 roots


def batch_rate(nof_prb, config_idx, flags, warmup, repeats):
    cfgs = [abi.prach_cfg(nof_prb=nof_prb, config_idx=config_idx, freq_offset=(nof_prb - 6) // 2, preamble_idx=i, **CELL)
            for i in range(64)]
    b = abi.PrachBatch(cfgs, flags=flags)
    d_iq = torch.zeros(2 * b.iq_samples, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: b.run(d_iq.data_ptr(), st), warmup, repeats)
    med, lo, hi = float(np.median(ms)), float(ms[0]), float(ms[-1])
    fill = float(np.median(timed(lambda: d_iq.fill_(1.0), warmup, repeats)))
    gb = 8 * b.iq_samples / 1e9
    out = {"nof_prb": nof_prb, "format": config_idx // 16, "single_residue": bool(flags), "preambles": 64,
           "iq_mbytes": gb * 1e3, "median_ms": med, "min_ms": lo, "max_ms": hi, "preambles_per_s": 64 / (med * 1e-3),
           "iq_gbytes_per_s": gb / (med * 1e-3), "fill_median_ms": fill, "fill_gbytes_per_s": gb / (fill * 1e-3),
           "fraction_of_fill_rate": fill / med}
    b.close()
    return out


def per_call(nof_prb, config_idx, repeats):
    rec = struct.pack("8i", nof_prb, config_idx, CELL["root_seq_idx"], CELL["high_speed"], CELL["zero_corr_zone"],
                      (nof_prb - 6) // 2, 5, 0) + struct.pack("2f", 0.3, 0.5)
    return run_harness("ue_prach_harness", rec, repeats, nof_prb=nof_prb, format=config_idx // 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--call-repeats", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [(6, 0), (6, 48), (100, 0), (100, 48)]
    r = {"device": need_gpu("prach_rate.py"),
         "batch": [batch_rate(prb, c, flags, a.warmup, a.repeats) for prb, c in shapes
                   for flags in (0, abi.PRACH_FLAG_SINGLE_RESIDUE)],
         "per_call": [per_call(prb, c, a.call_repeats) for prb, c in shapes]}
    report(r, a.out)


if __name__ == "__main__":
    main()
