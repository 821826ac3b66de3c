#!/usr/bin/env python3
"""Cost of the CSI feedback kernel on the GPU: a two-antenna batch of 20 MHz two-port subframes (one
transmitted subframe per antenna, replicated), one stream, MI_DL_FLAG_PROFILE.

After a warm-up each repetition runs the batch's front end (OFDM | CHEST: the chest stage's milliseconds come from
mi_dl_batch_stage_ms) and then mi_dl_csi_run between two HIP events.  Reported: csi_kernel's and chest_kernel's
milliseconds (median and min .. max), the bytes the CSI kernel must move -- per subframe the four pilot rows of 2
antennas x 2 ports (4 x 1200 x 4 x 8 B = 153.6 KB at 100 PRB) in and one record out -- the rate that makes, and the time
those bytes would take at the measured HBM copy rate (6.29 TB/s).  No target: the figures are a cost."""
import argparse
import ctypes as C

import numpy as np
import torch

from rate_common import need_gpu, report   # puts the repository root on sys.path
import bench
from rxdiv_rate import spread
from srsue_amd import abi

H = ((0.9, 0.3 + 0.2j), (-0.2 + 0.3j, 0.8))      # [antenna][port]
HBM_COPY_BYTES_PER_S = 6.29e12                   # measured float4 copy rate of the MI355X
S_OFDM, S_CHEST = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=int, default=12500, help="subframes of the batch")
    ap.add_argument("--prb", type=int, default=100)
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = need_gpu("csi_rate.py")
    dev = torch.device("cuda:0")
    cfg = abi.sf_cfg(cell_id=1, nof_prb=a.prb, nof_ports=2, sf_idx=1, cfi=1, tm=2, tbs=2216, Qm=2)
    tb = bench.tb_payload(0, cfg.tbs // 8)
    b = abi.Batch([cfg] * a.sf, profile=True, n_rx=2)
    d_iq = torch.empty(2 * 2 * b.iq_samples, dtype=torch.float32, device=dev)
    for ant in range(2):
        iq = abi.tx_subframe(cfg, tb, h=list(H[ant]), snr_db=a.snr, seed=0xC51 + ant)
        d_iq[2 * ant * b.iq_rx_stride:2 * (ant + 1) * b.iq_rx_stride].view(a.sf, -1).copy_(
            torch.from_numpy(iq).to(dev)[None, :])
    csi = abi.Csi(b)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(a.warmup):
        b.run_stages(S_OFDM | S_CHEST, d_iq.data_ptr(), st)
        csi.run(st)
    torch.cuda.synchronize()
    csi_ms, chest_ms = [], []
    for _ in range(a.repeats):
        b.profile_reset()
        b.run_stages(S_OFDM | S_CHEST, d_iq.data_ptr(), st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        csi.run(st)
        e1.record()
        e1.synchronize()
        csi_ms.append(e0.elapsed_time(e1))
        chest_ms.append(b.stage_ms()[0]["chest"])
    r0, r1 = csi.result(0), csi.result(a.sf - 1)
    in_bytes = a.sf * 4 * 12 * a.prb * 2 * 2 * 8
    out_bytes = a.sf * C.sizeof(abi.CsiResult)
    c, ch = spread(csi_ms), spread(chest_ms)
    out = {"device": name, "subframes": a.sf, "nof_prb": a.prb, "n_rx": 2, "ports": 2, "repeats": a.repeats,
           "csi_ms": c, "chest_ms": ch, "csi_over_chest": c["median"] / ch["median"],
           "csi_algo_bytes": in_bytes + out_bytes, "chest_algo_bytes": b.algo_bytes(abi.STAGES.index("chest")),
           "csi_gbytes_per_s": (in_bytes + out_bytes) / (c["median"] * 1e6),
           "hbm_bound_ms": (in_bytes + out_bytes) / HBM_COPY_BYTES_PER_S * 1e3,
           "csi_us_per_subframe": c["median"] * 1e3 / a.sf,
           "record": {"wideband_cqi": int(r0.cqi[0][0][0]), "pmi_r1": r0.pmi_r1, "cb_r2": r0.cb_r2, "ri_cl": r0.ri_cl,
                      "ri_ol": r0.ri_ol, "noise": r0.noise, "same_first_last": bytes(r0) == bytes(r1)}}
    csi.close()
    b.close()
    report(out, a.out)


if __name__ == "__main__":
    main()
