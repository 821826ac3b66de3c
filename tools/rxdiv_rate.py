#!/usr/bin/env python3
"""Cost of the second receive antenna on the GPU (receive diversity): the headline shard (bench.py
config 4: 12,500 subframes of 20 MHz TM1 MCS 28) and a 1,000-subframe TM2 one (config 3) decoded by a one-antenna
and by a two-antenna batch (mi_dl_batch_create_rx), one stream, MI_DL_FLAG_PROFILE.

After a warm-up the two batches run alternately in one process.  Per antenna count: the per-stage milliseconds of
mi_dl_batch_stage_ms (median and min .. max over the repetitions), the whole run's milliseconds and decoded Mbps, and
the bytes per second the rate de-matching stage (with the fused demap) achieves on mi_dl_batch_algo_bytes of the demap
and rate de-matching stages; then the two-antenna / one-antenna ratio of every stage.  Each antenna gets the same
transport blocks through its own flat channel with its own noise (mi_tx_subframe once per antenna).  There is no
target: the figures are a record."""
import argparse

import numpy as np
import torch

from rate_common import need_gpu, report   # puts the repository root on sys.path
import bench
from srsue_amd import abi


def make_inputs(cfgs, pool, n_rx, snr_db):
    tbs = [bench.tb_payload(i, cfgs[i].tbs // 8) for i in range(pool)]
    hs = ([1.0 + 0.0j, 0.6 - 0.5j], [-0.3 + 0.9j, 0.8 + 0.2j])
    iqs = [[abi.tx_subframe(cfgs[i], tbs[i], h=hs[a], snr_db=snr_db, seed=0xA5A5 + 2 * i + a) for i in range(pool)]
           for a in range(n_rx)]
    return iqs, tbs


def device_iq(b, iqs, dev):
    """the batch's IQ planes in HBM: the pool's subframes dealt to the batch's subframes (one bandwidth)"""
    B = len(b.cfgs)
    sfl = len(iqs[0][0])
    d_iq = torch.empty(2 * b.n_rx * b.iq_samples, dtype=torch.float32, device=dev)
    idx = torch.arange(B, device=dev) % len(iqs[0])
    for a in range(b.n_rx):
        d_pool = torch.from_numpy(np.stack(iqs[a])).to(dev)
        d_iq[2 * a * b.iq_rx_stride:2 * (a + 1) * b.iq_rx_stride].view(B, sfl).copy_(d_pool[idx])
        del d_pool
    return d_iq


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1])}


def measure(config, n_sf, pool, snr_db, max_its, warmup, repeats, dev):
    cfgs = bench.config_cfgs(config, n_sf, 0)
    pool = min(pool, n_sf)
    iqs, tbs = make_inputs(cfgs, pool, 2, snr_db)
    st = torch.cuda.current_stream().cuda_stream
    runs = {}
    for n_rx in (1, 2):
        b = abi.Batch(cfgs, max_its=max_its, profile=True, compact_ce=True, n_rx=n_rx)
        runs[n_rx] = (b, device_iq(b, iqs, dev))
    for _ in range(warmup):
        for b, d in runs.values():
            b.run(d.data_ptr(), st)
    torch.cuda.synchronize()
    stage = {1: [], 2: []}
    total = {1: [], 2: []}
    for _ in range(repeats):
        for n_rx, (b, d) in runs.items():       # alternating: both see the same clocks and neighbours
            b.profile_reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.run(d.data_ptr(), st)
            e1.record()
            e1.synchronize()
            total[n_rx].append(e0.elapsed_time(e1))
            stage[n_rx].append(b.stage_ms()[0])
    out = {"config": config, "subframes": n_sf, "snr_db": snr_db, "max_its": max_its, "repeats": repeats}
    for n_rx, (b, d) in runs.items():
        crc = b.download(abi.BUF_TB_CRC, np.uint32)[:n_sf]
        pay = b.download(abi.BUF_PAYLOAD, np.uint8)
        bad = sum(int(not np.array_equal(b.payload(i, pay), tbs[i % pool])) for i in range(n_sf) if crc[i])
        bits = float(sum(c.tbs for c, o in zip(cfgs, crc) if o))
        ms = {k: spread([s[k] for s in stage[n_rx]]) for k in abi.STAGES}
        tot = spread(total[n_rx])
        fused_bytes = b.algo_bytes(abi.STAGES.index("demap")) + b.algo_bytes(abi.STAGES.index("rm"))
        out[f"n_rx{n_rx}"] = {"stage_ms": ms, "run_ms": tot, "tb_crc_ok": int(crc.sum()), "payload_mismatch": bad,
                              "mbps": bits / (tot["median"] * 1e3),
                              "algo_bytes": {k: b.algo_bytes(i) for i, k in enumerate(abi.STAGES)},
                              "rm_fused_gbytes_per_s": fused_bytes / (ms["rm"]["median"] * 1e6),
                              "device_bytes": b.device_bytes}
    one, two = out["n_rx1"], out["n_rx2"]
    out["ratio_2_over_1"] = {k: (two["stage_ms"][k]["median"] / one["stage_ms"][k]["median"]
                                 if one["stage_ms"][k]["median"] > 0 else None) for k in abi.STAGES}
    out["ratio_2_over_1"]["run"] = two["run_ms"]["median"] / one["run_ms"]["median"]
    for b, d in runs.values():
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=int, default=12500, help="subframes of the TM1 shard (bench.py config 4)")
    ap.add_argument("--sf-tm2", type=int, default=1000, help="subframes of the TM2 shard (bench.py config 3)")
    ap.add_argument("--pool", type=int, default=64, help="distinct synthetic subframes per antenna")
    ap.add_argument("--snr", type=float, default=30.0)
    ap.add_argument("--max-its", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = need_gpu("rxdiv_rate.py")
    dev = torch.device("cuda:0")
    r = {"device": name,
         "shards": [measure(4, a.sf, a.pool, a.snr, a.max_its, a.warmup, a.repeats, dev),
                    measure(3, a.sf_tm2, a.pool, a.snr, a.max_its, a.warmup, a.repeats, dev)]}
    report(r, a.out)


if __name__ == "__main__":
    main()
