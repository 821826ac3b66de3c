#!/usr/bin/env python3
"""PUCCH encode rates on the GPU (PUCCH): transmissions per second of mi_pucch_batch_run for small and
large batches (one launch, all six formats mixed, HIP events around the call), and microseconds per call of the
per-TTI mi_ue_ul_pucch_encode (host clock inside tests/c/ue_pucch_harness: plan, table upload, kernel, IQ
download and copy-out).

Warm-up, then repeated timed calls; reports the median and the spread (min .. max).  There is no earlier path to
compare with: the figures are a record."""
import argparse
import struct

import numpy as np
import torch

from rate_common import need_gpu, report, run_harness, stats, timed   # puts the repository root on sys.path
from srsue_amd import abi


def batch_rate(n, nof_prb, warmup, repeats):
    cfgs = []
    for i in range(n):
        fmt = i % 6
        cfgs.append(abi.pucch_cfg(cell_id=i % 504, nof_prb=nof_prb, sf_idx=i % 10, rnti=1 + i % 65000, format=fmt,
                                  n_pucch=i % 12 if fmt >= abi.PUCCH_2 else i % 36, n_rb_2=1, group_hopping=i & 1,
                                  shortened=int(fmt < abi.PUCCH_2 and i % 5 == 0), cqi_len=4 if fmt >= abi.PUCCH_2 else 0))
    b = abi.PucchBatch(cfgs)
    rng = np.random.default_rng(1)
    words = (rng.integers(0, 4, n) | (rng.integers(0, 16, n) << 8)).astype(np.int32)
    d_uci = torch.from_numpy(words).cuda()
    d_iq = torch.zeros(2 * b.iq_samples, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: b.run(d_uci.data_ptr(), d_iq.data_ptr(), st), warmup, repeats)
    out = dict(stats(ms, n), transmissions=n, nof_prb=nof_prb, iq_gbytes_per_s=float(8 * b.iq_samples / (np.median(ms) * 1e6)))
    b.close()
    return out


def per_tti(nof_prb, repeats):
    """ACK (format 1a), ACK + CQI (format 2a) and SR (format 1), each repeated `repeats` times"""
    calls = [(14, 7, 1, 1, 0, 0), (25, 7, 1, 0, 0, 4), (36, 0, 0, 0, 1, 0)]
    rec = struct.pack("16i", 1, nof_prb, len(calls), 0, 0, 1, 0, 1, 0, 0, 0, 11, 3, 29, 0x46, 0) + struct.pack("f", 0.0)
    for c in calls:
        rec += struct.pack("6i", *c) + bytes([1, 0, 1, 1] + [0] * 60)
    return run_harness("ue_pucch_harness", rec, repeats, nof_prb=nof_prb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--tti-repeats", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = {"device": need_gpu("pucch_rate.py"),
         "batch": [batch_rate(n, prb, a.warmup, a.repeats) for prb in (6, 100) for n in a.batches],
         "per_tti": [per_tti(prb, a.tti_repeats) for prb in (6, 100)]}
    report(r, a.out)


if __name__ == "__main__":
    main()
