#!/usr/bin/env python3
"""Acquisition rates on the GPU (cell acquisition): PBCH candidates per second (4-frame candidates,
soft bits + blind decode, one launch per stage) and half-frame windows searched per second (cell search: all
lags x 3 PSS roots + SSS per window and root, one launch per stage).

Warm-up, then repeated timed calls; reports the median and the spread (min .. max).  PBCH: HIP events around the
two kernels, and around OFDM + channel estimation + the two kernels.  Cell search: host clock around the
synchronous call (it ends in the result download, and includes the host's per-chunk reduction).  There is no
earlier path to compare with: the figures are a record."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srsue_amd import abi  # noqa: E402


def stats(ms, n):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms[0]), "max_ms": float(ms[-1]),
            "per_s_median": float(n / (np.median(ms) * 1e-3)), "per_s_min": float(n / (ms[-1] * 1e-3)),
            "per_s_max": float(n / (ms[0] * 1e-3))}


def pbch_rate(n_cand, warmup, repeats):
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, 24).astype(np.uint8)
    frames = []
    for ph in range(4):     # one BCH TTI of a 2-port cell at 5 dB, reused by every candidate
        cfg = abi.sf_cfg(cell_id=7, nof_prb=6, nof_ports=2, sf_idx=0, cfi=2, tbs=208, Qm=2)
        iq = abi.tx_subframe(cfg, np.zeros(26, np.uint8), h=[0.8 + 0.3j, -0.4 + 0.5j], snr_db=300.0)
        abi.tx_pbch(7, 6, 2, bits, ph, iq, h=[0.8 + 0.3j, -0.4 + 0.5j])
        frames.append(iq + rng.normal(0, np.sqrt(10 ** -0.5 / 2), len(iq)).astype(np.float32))
    cfgs = [abi.sf_cfg(cell_id=7, nof_prb=6, nof_ports=2, sf_idx=0, cfi=2, tbs=208, Qm=2)] * (4 * n_cand)
    b = abi.Batch(cfgs, max_its=1)
    flat = np.zeros(2 * b.iq_samples, np.float32)
    for i in range(4 * n_cand):
        o = 2 * b.iq_offset(i)
        flat[o:o + len(frames[i % 4])] = frames[i % 4]
    d = torch.from_numpy(flat).cuda()
    st = torch.cuda.current_stream().cuda_stream
    p = abi.Pbch(b)
    p.set_candidates([[4 * c, 4 * c + 1, 4 * c + 2, 4 * c + 3] for c in range(n_cand)])
    out = {"candidates": n_cand, "frames": 4 * n_cand, "decodes": p.n_jobs}

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    b.run_stages(3, d.data_ptr(), st)
    out["pbch"] = stats(timed(lambda: p.run(st, mask=3)), n_cand)
    out["front_and_pbch"] = stats(timed(lambda: (b.run_stages(3, d.data_ptr(), st), p.run(st, mask=3))), n_cand)
    found = sum(p.result(c) is not None for c in range(n_cand))
    out["found"] = found
    assert found == n_cand, "the rate input is meant to decode"
    p.close()
    b.close()
    return out


def search_rate(n_win, warmup, repeats):
    half = abi.CellSearch.HALF
    rng = np.random.default_rng(2)
    frame = []
    for i in range(10):
        cfg = abi.sf_cfg(cell_id=301, nof_prb=6, sf_idx=i, cfi=2, tbs=208, Qm=2)
        iq = abi.tx_subframe(cfg, np.zeros(26, np.uint8), snr_db=300.0)
        abi.tx_sync(301, 6, i, iq)
        frame.append(iq)
    frame = np.concatenate(frame)
    x = np.tile(frame, n_win // 2 + 1)[:2 * (n_win * half + 128)]
    x = x + rng.normal(0, np.sqrt(0.05), len(x)).astype(np.float32)      # 10 dB
    d = torch.from_numpy(x).cuda()
    cs = abi.CellSearch()
    offs = [w * half for w in range(n_win)]
    st = torch.cuda.current_stream().cuda_stream
    ms = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = cs.run(d.data_ptr(), offs, stream_ptr=st)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert res[1]["found"] and res[1]["cell_id"] == 301 and res[1]["mode"] == 1.0, res
    cs.close()
    return {"windows": n_win, "pss_jobs": n_win * 450, "search": stats(ms, n_win)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("acq_rate.py needs a GPU")
    r = {"device": torch.cuda.get_device_name(0), "pbch": pbch_rate(a.candidates, a.warmup, a.repeats),
         "cellsearch": search_rate(a.windows, a.warmup, a.repeats)}
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
