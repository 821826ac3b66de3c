#!/usr/bin/env python3
"""Cost of two-layer spatial multiplexing on the GPU (spatial multiplexing): a batch of 20 MHz TM3 codeword
pairs (64QAM / 64QAM, one transmitted pair replicated) beside rxdiv_rate.py's two-antenna TM1 batch (bench.py config 4)
of the same subframe count, one stream, MI_DL_FLAG_PROFILE, both in one process.

After a warm-up the two batches run alternately.  Per batch: the per-stage milliseconds of mi_dl_batch_stage_ms
(median and min .. max over the repetitions), the whole run's milliseconds and decoded Mbps.  A batch with pairs is
never fused: its DEMAP stage (demap_kernel's empty pass plus sm_detect_kernel) writes the LLR stream of both codewords
and its RM stage reads it, so `unfused_over_fused` -- its DEMAP + RM time over the TM1 batch's fused RM time -- is what
the LLR stream costs, and `detect_gbytes_per_s` is the DEMAP stage on the bytes it must move (per RE 2 grid values and
4 estimates in, Qm0 + Qm1 floats out).  The two batches are different workloads: the figures are a cost, with no
target."""
import argparse

import numpy as np
import torch

from rate_common import need_gpu, report   # puts the repository root on sys.path
import bench
from rxdiv_rate import device_iq, make_inputs, spread
from srsue_amd import abi

H = ((0.9, 0.3 + 0.2j), (-0.2 + 0.3j, 0.8))      # [antenna][port], |det| = 0.84


def sm_pair(tbs, qm, tm=3, pmi=0):
    return [abi.sf_cfg(cell_id=1, nof_prb=100, nof_ports=2, sf_idx=1, cfi=1, tm=tm, tbs=tbs, Qm=qm, cw=q, pmi=pmi) for q in range(2)]


def timed_runs(runs, warmup, repeats):
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        for b, d in runs.values():
            b.run(d.data_ptr(), st)
    torch.cuda.synchronize()
    stage = {k: [] for k in runs}
    total = {k: [] for k in runs}
    for _ in range(repeats):
        for k, (b, d) in runs.items():          # alternating: both see the same clocks and neighbours
            b.profile_reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.run(d.data_ptr(), st)
            e1.record()
            e1.synchronize()
            total[k].append(e0.elapsed_time(e1))
            stage[k].append(b.stage_ms()[0])
    return stage, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=int, default=12500, help="physical subframes of each batch")
    ap.add_argument("--tbs", type=int, default=36696, help="transport block size of each codeword")
    ap.add_argument("--snr", type=float, default=30.0)
    ap.add_argument("--max-its", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only-sm", action="store_true", help="run the pair batch alone (a kernel trace of its own)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = need_gpu("sm_rate.py")
    dev = torch.device("cuda:0")
    pair = sm_pair(a.tbs, 6)
    tbs = [bench.tb_payload(q, a.tbs // 8) for q in range(2)]
    sm_iqs = [[abi.tx_subframe_sm(pair, tbs[0], tbs[1], h=list(H[ant]), snr_db=a.snr, seed=0x5A5A + ant)] for ant in range(2)]
    runs = {}
    b = abi.Batch(pair * a.sf, max_its=a.max_its, profile=True, n_rx=2)
    d_iq = torch.empty(2 * 2 * b.iq_samples, dtype=torch.float32, device=dev)
    for ant in range(2):
        d_iq[2 * ant * b.iq_rx_stride:2 * (ant + 1) * b.iq_rx_stride].view(a.sf, -1).copy_(
            torch.from_numpy(sm_iqs[ant][0]).to(dev)[None, :])
    runs["sm"] = (b, d_iq)
    if not a.only_sm:
        cfgs = bench.config_cfgs(4, a.sf, 0)
        iqs, tm1_tbs = make_inputs(cfgs, min(64, a.sf), 2, a.snr)
        b1 = abi.Batch(cfgs, max_its=a.max_its, profile=True, compact_ce=True, n_rx=2)
        runs["tm1_n_rx2"] = (b1, device_iq(b1, iqs, dev))
    stage, total = timed_runs(runs, a.warmup, a.repeats)
    out = {"device": name, "subframes": a.sf, "snr_db": a.snr, "max_its": a.max_its, "repeats": a.repeats,
           "sm_tbs_per_codeword": a.tbs}
    for k, (bb, _) in runs.items():
        crc = bb.download(abi.BUF_TB_CRC, np.uint32)
        pay = bb.download(abi.BUF_PAYLOAD, np.uint8)
        n = len(bb.cfgs)
        want = (lambda i: tbs[i % 2]) if k == "sm" else (lambda i: tm1_tbs[i % len(tm1_tbs)])
        bad = sum(int(not np.array_equal(bb.payload(i, pay), want(i))) for i in range(n) if crc[i])
        bits = float(sum(c.tbs for c, o in zip(bb.cfgs, crc) if o))
        ms = {s: spread([x[s] for x in stage[k]]) for s in abi.STAGES}
        tot = spread(total[k])
        out[k] = {"stage_ms": ms, "run_ms": tot, "entries": n, "tb_crc_ok": int(crc.sum()), "payload_mismatch": bad,
                  "mbps": bits / (tot["median"] * 1e3),
                  "algo_bytes": {s: bb.algo_bytes(i) for i, s in enumerate(abi.STAGES)}, "device_bytes": bb.device_bytes}
    sm = out["sm"]
    nre = abi.pdsch_G(pair[0]) // 6
    det_bytes = a.sf * nre * (6 * 8 + (6 + 6) * 4)
    sm["detect_bytes"] = det_bytes
    sm["detect_gbytes_per_s"] = det_bytes / (sm["stage_ms"]["demap"]["median"] * 1e6)
    if not a.only_sm:
        one = out["tm1_n_rx2"]
        out["sm_over_tm1"] = {s: (sm["stage_ms"][s]["median"] / one["stage_ms"][s]["median"]
                                  if one["stage_ms"][s]["median"] > 0 else None) for s in abi.STAGES}
        out["sm_over_tm1"]["run"] = sm["run_ms"]["median"] / one["run_ms"]["median"]
        out["unfused_over_fused"] = (sm["stage_ms"]["demap"]["median"] + sm["stage_ms"]["rm"]["median"]) / \
            one["stage_ms"]["rm"]["median"]
    for bb, _ in runs.values():
        bb.close()
    report(out, a.out)


if __name__ == "__main__":
    main()
