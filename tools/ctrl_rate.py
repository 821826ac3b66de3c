#!/usr/bin/env python3
"""Cost of one DL control run of a batch on the GPU: 20 MHz subframes (one transmitted subframe per
antenna, replicated; each subframe's search runs for its own cfg.rnti), one stream.

Three control objects are timed after the batch's front end (OFDM | CHEST) has left grid and estimates in HBM:
  one_antenna        a one-antenna batch (mi_dl_ctrl_create)
  two_plane0         a two-antenna batch read as before: plane 0 alone (mi_dl_ctrl_create)
  two_combined       the same batch with MI_CTRL_FLAG_RX_COMBINE
each stage by stage (PCFICH, PDCCH soft bits, blind search, PHICH: one launch between two HIP events) and whole (the
four launches of mi_dl_ctrl_run), median and min .. max over the repeats.  --only one_antenna times the first alone;
with SRSUE_AMD_LIB pointing at a library built from another commit that is the A/B of the one-antenna step.
No target: the figures are a cost."""
import argparse

import torch

from rate_common import need_gpu, report, timed   # puts the repository root on sys.path
import bench
from rxdiv_rate import spread
from srsue_amd import abi

H = ((0.9, 0.3 + 0.2j), (-0.2 + 0.3j, 0.8))      # [antenna][port]
S_OFDM, S_CHEST = 1, 2
STAGES = (("pcfich", abi.Ctrl.PCFICH), ("pdcch_llr", abi.Ctrl.LLR), ("search", abi.Ctrl.SEARCH), ("phich", abi.Ctrl.PHICH),
          ("whole", 15))


def front(cfg, n_sf, n_rx, snr, dev):
    """a batch of n_sf copies of cfg after OFDM | CHEST (kept alive with its samples)"""
    tb = bench.tb_payload(0, cfg.tbs // 8)
    b = abi.Batch([cfg] * n_sf, n_rx=n_rx)
    d_iq = torch.empty(2 * n_rx * b.iq_samples, dtype=torch.float32, device=dev)
    for ant in range(n_rx):
        iq = abi.tx_subframe(cfg, tb, h=list(H[ant][:cfg.nof_ports]), snr_db=snr, seed=0xC7A + ant)
        d_iq[2 * ant * b.iq_samples:2 * (ant + 1) * b.iq_samples].view(n_sf, -1).copy_(torch.from_numpy(iq).to(dev)[None, :])
    b.run_stages(S_OFDM | S_CHEST, d_iq.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return b, d_iq


def measure(ctl, warmup, repeats):
    st = torch.cuda.current_stream().cuda_stream
    return {name: spread(timed(lambda m=mask: ctl.run(st, mask=m), warmup, repeats)) for name, mask in STAGES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=int, default=12500, help="subframes of the batch")
    ap.add_argument("--prb", type=int, default=100)
    ap.add_argument("--ports", type=int, default=1)
    ap.add_argument("--cfi", type=int, default=1)
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--only", choices=["one_antenna"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = need_gpu("ctrl_rate.py")
    dev = torch.device("cuda:0")
    cfg = abi.sf_cfg(cell_id=1, nof_prb=a.prb, nof_ports=a.ports, sf_idx=1, cfi=a.cfi, tbs=2216, Qm=2)
    out = {"device": name, "subframes": a.sf, "nof_prb": a.prb, "ports": a.ports, "cfi": a.cfi, "repeats": a.repeats}
    b1, iq1 = front(cfg, a.sf, 1, a.snr, dev)
    c = abi.Ctrl(b1, phich_ng=2)
    out["one_antenna"] = measure(c, a.warmup, a.repeats)
    out["cfi_ok"] = c.result(0)[0] == a.cfi and c.result(a.sf - 1)[0] == a.cfi
    c.close()
    b1.close()
    del iq1
    if a.only is None:
        b2, iq2 = front(cfg, a.sf, 2, a.snr, dev)
        for key, combine in (("two_plane0", False), ("two_combined", True)):
            c = abi.Ctrl(b2, phich_ng=2, combine=combine)
            out[key] = measure(c, a.warmup, a.repeats)
            out["jobs_per_subframe"] = c.n_jobs / a.sf
            out["cfi_ok"] = out["cfi_ok"] and c.result(0)[0] == a.cfi
            c.close()
        out["combined_over_plane0"] = {k: out["two_combined"][k]["median"] / out["two_plane0"][k]["median"] for k, _ in STAGES}
        b2.close()
    report(out, a.out)


if __name__ == "__main__":
    main()
