"""What the *_rate.py tools share: the warm-up + HIP-event timing loop, its statistics, the harness call and the
result line."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    """milliseconds of each of `repeats` calls of fn (HIP events around the call), sorted, after `warmup` calls"""
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
    return np.sort(np.asarray(ms))


def stats(ms, n):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms[0]), "max_ms": float(ms[-1]),
            "per_s_median": float(n / (np.median(ms) * 1e-3)), "per_s_min": float(n / (ms[-1] * 1e-3)),
            "per_s_max": float(n / (ms[0] * 1e-3))}


def run_harness(name, records, repeats, **extra):
    """writes `records` (bytes) as the input file of tests/c/<name>, runs it `repeats` times per call and returns
    the JSON of its last output line, with `extra` added"""
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(records)
        out = subprocess.check_output([os.path.join(ROOT, "tests", "c", name), fin, fout, str(repeats)], timeout=300)
    return dict(json.loads(out.decode().strip().splitlines()[-1]), **extra)


def need_gpu(tool):
    if not torch.cuda.is_available():
        sys.exit(tool + " needs a GPU")
    return torch.cuda.get_device_name(0)


def report(r, out):
    line = json.dumps(r)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
