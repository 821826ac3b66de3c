"""GPU: the PRACH preamble transmitter (srsue_amd/csrc/prach.hip through mi_prach_batch_* and mi_prach_init / _gen /
_gen_cfo) against the independent reference of tests/prach_ref.py: IQ parity for formats 0-3, both sets and every
polyphase factor L, every output sample written, the frequency shift and scale, the reference detector on the
product's IQ, plan reuse on a side stream, the single-residue variant, the per-call path in srsUE's call order
(tests/c/ue_prach_harness.c) and the rejections.

Measured on one MI355X (bound TOL = 1e-4, the project's IQ bound): worst RMS-relative error 3.5e-7 over the 137
transmissions (the 75 PRB one), 3.6e-7 with a frequency shift and a scale, 3.5e-7 for mi_prach_gen_cfo."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import prach_ref as R
from srsue_amd import abi

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "ue_prach_harness")
TOL = 1e-4   # TOL of tests/test_gpu_pucch.py


def cfg(nof_prb=6, config_idx=0, root_seq_idx=22, zero_corr_zone=12, high_speed=0, freq_offset=0, preamble_idx=0):
    return dict(nof_prb=nof_prb, config_idx=config_idx, root_seq_idx=root_seq_idx, zero_corr_zone=zero_corr_zone,
                high_speed=high_speed, freq_offset=freq_offset, preamble_idx=preamble_idx)


CELL6 = [cfg(preamble_idx=i) for i in range(64)]            # 6 PRB (L = 1): N_CS = 119, 7 shifts per root, 10 roots
CASES = CELL6 + [
    cfg(config_idx=16, preamble_idx=9), cfg(config_idx=32, preamble_idx=17), cfg(config_idx=48, preamble_idx=30),
    cfg(root_seq_idx=264, zero_corr_zone=4, high_speed=1, preamble_idx=7),     # u = 5: d_u = 168 < 839 / 3
    cfg(root_seq_idx=384, zero_corr_zone=4, high_speed=1, preamble_idx=5),     # u = 3: d_u = 280 >= 839 / 3
    cfg(nof_prb=15, freq_offset=5, preamble_idx=11),                           # L = 2
] + [cfg(nof_prb=15, root_seq_idx=800, zero_corr_zone=0, freq_offset=9, preamble_idx=i) for i in range(64)] + [
    cfg(nof_prb=75, root_seq_idx=455, zero_corr_zone=7, freq_offset=30, preamble_idx=40),   # L = 12
    cfg(nof_prb=100, config_idx=48, root_seq_idx=837, zero_corr_zone=9, freq_offset=94, preamble_idx=63),  # 70,176 samples
    cfg(nof_prb=100, root_seq_idx=100, zero_corr_zone=1, freq_offset=0, preamble_idx=2),    # k0 < 0
]
CELL15 = slice(70, 134)
# transmissions that get a frequency shift and a scale (subcarriers of 15 kHz; amplitude)
SHIFTED = {3: (0.37, 0.5), 64: (-0.81, 2.0), 66: (0.05, 1.5), 68: (1.25, 0.25), 69: (-0.4, 3.0), 100: (0.6, 1.0),
           134: (0.9, 0.7), 135: (-0.33, 1.75), 136: (0.71, 1.0)}


def rel_err(a, b):
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / np.sqrt(np.mean(np.abs(b) ** 2)))


def run_batch(b, stream=None, fill=0.0, cfo=None, scale=None):
    d_iq = torch.full((2 * b.iq_samples,), fill, dtype=torch.float32, device="cuda")
    d_cfo = None if cfo is None else torch.from_numpy(np.asarray(cfo, np.float32)).cuda()
    d_scale = None if scale is None else torch.from_numpy(np.asarray(scale, np.float32)).cuda()
    torch.cuda.synchronize()
    s = stream or torch.cuda.current_stream()
    b.run(d_iq.data_ptr(), s.cuda_stream, None if d_cfo is None else d_cfo.data_ptr(),
          None if d_scale is None else d_scale.data_ptr())
    s.synchronize()
    return d_iq.cpu().numpy()


def piece(b, iq, i, r):
    o = b.iq_offset(i)
    return iq.view(np.complex64)[o:o + r["N_cp"] + r["N_seq"]]


@pytest.fixture(scope="module")
def generated(built):
    b = abi.PrachBatch([abi.prach_cfg(**c) for c in CASES])
    res = [R.resource(**c) for c in CASES]
    iq = run_batch(b, fill=7.0)
    want = [R.iq(c) for c in CASES]
    return b, res, iq, want


def test_cases_cover_what_they_claim():
    assert R.d_u(R.resource(**CASES[67])["u"]) < R.NZC / 3 <= R.d_u(R.resource(**CASES[68])["u"])
    assert len({R.resource(**c)["u"] for c in CELL6}) == 10
    cell15 = [R.resource(**c) for c in CASES[CELL15]]
    assert len({r["u"] for r in cell15}) == 64 and all(r["C_v"] == 0 and r["n_roots"] == 64 for r in cell15)
    assert sorted({R.resource(**c)["N_ifft"] // 1536 for c in CASES}) == [1, 2, 12, 16]
    big = R.resource(**CASES[135])
    assert big["N_cp"] + big["N_seq"] == 70176
    # the 839 bins straddle DC (they wrap in the N_ifft grid and in the 1536-point one) at 6 and 15 PRB; at 100 PRB
    # with offset 0 they lie in the negative half
    for i in (0, 69):
        r = R.resource(**CASES[i])
        assert r["first_bin"] + R.NZC > r["N_ifft"] and r["first_bin"] % 1536 + R.NZC > 1536
    assert R.resource(**CASES[136])["first_bin"] > 24576 // 2
    assert [R.resource(**CASES[i])["format"] for i in (64, 65, 66)] == [1, 2, 3]


def test_batch_layout_and_resources_match_reference(generated):
    b, res, _, _ = generated
    off = 0
    for i, r in enumerate(res):
        assert b.iq_offset(i) == off
        off += r["N_cp"] + r["N_seq"]
        got = b.resource(i)
        assert {f: getattr(got, f) for f in abi.PRACH_RES_FIELDS} == r, i
    assert b.iq_samples == off


def test_batch_iq_matches_reference_and_every_sample_is_written(generated):
    b, res, iq, want = generated
    assert not np.any(iq == 7.0)
    errs = [rel_err(piece(b, iq, i, r), want[i]) for i, r in enumerate(res)]
    print("worst rel_err", max(errs), "at", int(np.argmax(errs)))
    for i, e in enumerate(errs):
        assert e < TOL, (i, e)


def test_frequency_shift_and_scale(generated):
    b, res, iq, _ = generated
    cfo, scale = np.zeros(len(CASES), np.float32), np.ones(len(CASES), np.float32)
    for i, (f, g) in SHIFTED.items():
        cfo[i], scale[i] = f, g
    got = run_batch(b, fill=7.0, cfo=cfo, scale=scale)
    assert not np.any(got == 7.0)
    errs = {}
    for i, r in enumerate(res):
        if i in SHIFTED:
            errs[i] = rel_err(piece(b, got, i, r), R.iq(CASES[i], float(cfo[i]), float(scale[i])))
        else:   # zero shift, unit scale: the same samples as with no arrays at all
            assert np.array_equal(piece(b, got, i, r), piece(b, iq, i, r)), i
    print("worst rel_err with cfo and scale", max(errs.values()))
    for i, e in errs.items():
        assert e < TOL, (i, e)
    # one array without the other
    only = run_batch(b, cfo=cfo)
    for i in (3, 136):
        assert rel_err(piece(b, only, i, res[i]), R.iq(CASES[i], float(cfo[i]), 1.0)) < TOL


def test_reference_detector_recovers_every_preamble_and_the_delay(generated):
    b, res, iq, _ = generated
    for i, r in enumerate(res):
        s = piece(b, iq, i, r).astype(complex)
        delay = 1 + i % 5
        rx = np.concatenate([np.zeros(delay), s])[:len(s)]
        assert R.detect(rx, CASES[i]) == (CASES[i]["preamble_idx"], delay), i


def test_same_plan_twice_on_a_side_stream_is_bit_identical(generated):
    b, _, iq, _ = generated
    side = torch.cuda.Stream()
    one = run_batch(b, stream=side, fill=7.0)
    two = run_batch(b, stream=side, fill=-3.0)
    assert np.array_equal(one, two) and np.array_equal(one, iq)


def test_single_residue_variant_is_bit_identical(generated):
    """a workgroup per residue (strided writes) computes the same transforms as a workgroup per 2 or 4 residues"""
    b, res, iq, _ = generated
    pick = [69, 70, 134, 135, 136]
    s = abi.PrachBatch([abi.prach_cfg(**CASES[i]) for i in pick], flags=abi.PRACH_FLAG_SINGLE_RESIDUE)
    out = run_batch(s, fill=7.0)
    assert not np.any(out == 7.0)
    for k, i in enumerate(pick):
        assert np.array_equal(piece(s, out, k, res[i]), piece(b, iq, i, res[i])), i


BAD = [dict(nof_prb=7), dict(config_idx=30), dict(config_idx=64), dict(root_seq_idx=838), dict(zero_corr_zone=16),
       dict(zero_corr_zone=15, high_speed=1), dict(freq_offset=1), dict(preamble_idx=64)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_batch_create_rejects(built, bad):
    with pytest.raises(RuntimeError, match="PRACH"):
        abi.PrachBatch([abi.prach_cfg(**cfg()), abi.prach_cfg(**dict(cfg(), **bad))])


# ---- the per-call path ---------------------------------------------------------------------------------------
def run_harness(c, cfo_preamble=0, cfo=0.0, scale=1.0):
    """-> (init ret, N_seq, N_cp), [64 x (ret, samples)], send_tti table [64][20], (gen_cfo ret, samples)"""
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("8i", c["nof_prb"], c["config_idx"], c["root_seq_idx"], c["high_speed"],
                                c["zero_corr_zone"], c["freq_offset"], cfo_preamble, 0))
            f.write(struct.pack("2f", cfo, scale))
        subprocess.check_call([HARNESS, fin, fout], timeout=120)
        raw = open(fout, "rb").read()
    head = struct.unpack_from("3i", raw, 0)
    if head[0]:
        assert len(raw) == 12
        return head, None, None, None
    n, pos, gens = head[1] + head[2], 12, []
    for _ in range(64):
        gens.append((struct.unpack_from("i", raw, pos)[0], np.frombuffer(raw, np.complex64, n, pos + 4)))
        pos += 4 + 8 * n
    table = np.frombuffer(raw, np.uint8, 64 * 20, pos).reshape(64, 20)
    pos += 64 * 20
    last = (struct.unpack_from("i", raw, pos)[0], np.frombuffer(raw, np.complex64, n, pos + 4))
    assert pos + 4 + 8 * n == len(raw)
    return head, gens, table, last


@pytest.fixture(scope="module")
def per_call(built):
    assert os.path.exists(HARNESS)
    return run_harness(CASES[0], cfo_preamble=41, cfo=-0.62, scale=0.8)


def test_per_call_lengths_and_preambles_equal_the_batch(per_call, generated):
    b, res, iq, _ = generated
    head, gens, _, _ = per_call
    assert head == (0, res[0]["N_seq"], res[0]["N_cp"])
    for i, (ret, s) in enumerate(gens):
        assert ret == 0 and np.array_equal(s, piece(b, iq, i, res[i])), i


def test_per_call_gen_cfo_and_send_tti(per_call):
    _, _, table, (ret, s) = per_call
    assert ret == 0
    e = rel_err(s, R.iq(CASES[41], np.float32(-0.62), np.float32(0.8)))
    print("gen_cfo rel_err", e)
    assert e < TOL
    assert table.tolist() == [[R.send_tti(c, t) for t in range(20)] for c in range(64)]


def test_per_call_format_3_at_20_mhz(built):
    """the largest preamble through the per-call path: every preamble of the cell against the reference"""
    c = cfg(nof_prb=100, config_idx=48, root_seq_idx=600, zero_corr_zone=10, freq_offset=47)
    head, gens, _, (ret, s) = run_harness(c, cfo_preamble=63, cfo=0.45, scale=1.0)
    assert head == (0, 2 * 24576, 21024) and ret == 0
    for i in (0, 31, 63):
        assert gens[i][0] == 0 and rel_err(gens[i][1], R.iq(dict(c, preamble_idx=i))) < TOL, i
    assert rel_err(s, R.iq(dict(c, preamble_idx=63), np.float32(0.45), 1.0)) < TOL


@pytest.mark.parametrize("bad", [dict(root_seq_idx=838), dict(zero_corr_zone=15, high_speed=1), dict(config_idx=62),
                                 dict(zero_corr_zone=16)])
def test_per_call_invalid_init_is_an_error(built, bad):
    head, gens, _, _ = run_harness(dict(CASES[0], **bad))
    assert head[0] != 0 and gens is None
