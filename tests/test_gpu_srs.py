"""GPU: the SRS transmitter (srsue_amd/csrc/srs.hip through mi_srs_batch_* and mi_ue_ul_srs_encode) against the
independent reference of tests/srs_ref.py: IQ parity, the reference receiver on the product's IQ, planned resources,
every output sample written and plan reuse on a side stream, the last-symbol-only form alone and over a shortened
PUCCH, scale and frequency shift, the rejections, and the per-TTI call with the power wrappers in srsUE's call order
(tests/c/ue_srs_harness.c)."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import pucch_ref as PR
import srs_ref as R
from srsue_amd import abi

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "ue_srs_harness")
TOL = 1e-4


def find_tti(cell_id, dss, want_v):
    """a subframe whose odd slot has c(ns) = want_v (sequence hopping, 5.5.1.4)"""
    return int(np.flatnonzero(R.c_seq(cell_id, dss)[1::2] == want_v)[0])


def make_cases():
    cases = []
    # 6 PRB, C_SRS 7: M_sc = 24 (tabulated), N / 2 = 64; all 30 groups via the cell id, both combs, every n_srs
    for u in range(30):
        cases.append(dict(nof_prb=6, bw_cfg=7, cell_id=u + 30 * (u % 5), k_tc=u % 2, n_srs=u % 8, tti=u, n_rrc=u % 24))
    # 15 PRB (odd N_RB in k0), C_SRS 5: M_sc = 72, the threshold of sequence hopping; v = 0 and v = 1
    for v in (0, 1):
        cases.append(dict(nof_prb=15, bw_cfg=5, cell_id=7, sh=1, dss=3, tti=40 + find_tti(7, 3, v), n_srs=3, k_tc=v))
    # 25 PRB, C_SRS 2, B = 1: M_sc = 24 inside a 24-PRB tree, hopping over its N_1 = 6 positions (T_SRS = 2)
    for k in range(6):
        cases.append(dict(nof_prb=25, bw_cfg=2, B=1, b_hop=0, n_rrc=9, cell_id=101, I_srs=0, tti=1000 + 2 * k, n_srs=k,
                          k_tc=k % 2))
    cases.append(dict(nof_prb=50, bw_cfg=0, B=2, n_rrc=7, k_tc=1, cell_id=222, n_srs=6, tti=77))
    # 75 PRB, C_SRS 0: N / 2 = 768, the radix-3 pass
    cases.append(dict(nof_prb=75, bw_cfg=0, cell_id=333, n_srs=1, tti=8))
    cases.append(dict(nof_prb=75, bw_cfg=0, cell_id=333, gh=1, n_srs=7, k_tc=1, tti=9))
    # 100 PRB, C_SRS 0: M_sc = 576, the largest; B = 3, b_hop = 0: the longest hopping product (2 . 2 . 6)
    cases.append(dict(nof_prb=100, bw_cfg=0, cell_id=444, n_srs=2, tti=5))
    cases.append(dict(nof_prb=100, bw_cfg=0, cell_id=444, gh=1, n_srs=5, k_tc=1, tti=6))
    for tti in (0, 14, 46):
        cases.append(dict(nof_prb=100, bw_cfg=0, B=3, b_hop=0, n_rrc=11, cell_id=500, gh=1, I_srs=1, tti=tti, n_srs=4))
    return [ref_cfg(c) for c in cases]


def ref_cfg(c):
    d = dict(cell_id=1, nof_prb=6, tti=0, bw_cfg=7, B=0, b_hop=3, n_rrc=0, k_tc=0, n_srs=0, I_srs=0, gh=0, sh=0, dss=0)
    d.update(c)
    return d


def product_cfg(d):
    return abi.srs_cfg(cell_id=d["cell_id"], nof_prb=d["nof_prb"], tti=d["tti"], bw_cfg=d["bw_cfg"], B=d["B"],
                       b_hop=d["b_hop"], n_rrc=d["n_rrc"], k_tc=d["k_tc"], n_srs=d["n_srs"], I_srs=d["I_srs"],
                       group_hopping=d["gh"], sequence_hopping=d["sh"], delta_ss=d["dss"])


def rel_err(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def run_batch(b, stream=None, fill=0.0, cfo=None, scale=None):
    d_iq = torch.full((2 * b.iq_samples,), fill, dtype=torch.float32, device="cuda")
    d_cfo = None if cfo is None else torch.from_numpy(np.asarray(cfo, np.float32)).cuda()
    d_scale = None if scale is None else torch.from_numpy(np.asarray(scale, np.float32)).cuda()
    torch.cuda.synchronize()
    s = stream or torch.cuda.current_stream()
    b.run(d_iq.data_ptr(), s.cuda_stream, d_cfo.data_ptr() if d_cfo is not None else None,
          d_scale.data_ptr() if d_scale is not None else None)
    s.synchronize()
    return d_iq.cpu().numpy()


def piece(b, iq, i, nof_prb):
    o = 2 * b.iq_offset(i)
    return iq[o:o + 2 * 15 * R.NFFT[nof_prb]]


def sym13(nof_prb):
    """float32 index of the first sample of symbol 13 (its CP) inside a subframe"""
    N = R.NFFT[nof_prb]
    return 2 * (14 * N - 144 * N // 2048)


@pytest.fixture(scope="module")
def encoded(built):
    refs = make_cases()
    b = abi.SrsBatch([product_cfg(d) for d in refs])
    iq = run_batch(b)
    want = [R.iq(d) for d in refs]
    return b, refs, iq, want


NCASES = 30 + 2 + 6 + 1 + 2 + 2 + 3


def test_case_list(encoded):
    _, refs, _, _ = encoded
    assert len(refs) == NCASES
    res = [R.resource(**d) for d in refs]
    assert sorted({int(r["u"][0]) for r in res[:30]}) == list(range(30))
    assert {d["n_srs"] for d in refs} == set(range(8)) and {d["k_tc"] for d in refs} == {0, 1}
    assert [int(r["v"][0]) for r in res[30:32]] == [0, 1] and int(res[30]["M_sc"][0]) == 72
    assert len({int(r["k0"][0]) - refs[32 + k]["k_tc"] for k, r in enumerate(res[32:38])}) == 6
    assert {int(r["M_sc"][0]) for r in res} >= {24, 72, 432, 576}
    assert {R.NFFT[d["nof_prb"]] // 2 for d in refs} == {64, 128, 256, 512, 768, 1024}


@pytest.mark.parametrize("i", range(NCASES))
def test_batch_iq_matches_reference(encoded, i):
    b, refs, iq, want = encoded
    e = rel_err(piece(b, iq, i, refs[i]["nof_prb"]), want[i])
    print("rel_err", i, e)
    assert e < TOL


def test_report_largest_error(encoded):
    b, refs, iq, want = encoded
    errs = [rel_err(piece(b, iq, i, d["nof_prb"]), want[i]) for i, d in enumerate(refs)]
    print("max rel_err", max(errs), "at", int(np.argmax(errs)))
    assert max(errs) < TOL


@pytest.mark.parametrize("i", range(NCASES))
def test_reference_receiver_on_product_iq(encoded, i):
    b, refs, iq, _ = encoded
    d = refs[i]
    m = R.receive(R.demod(piece(b, iq, i, d["nof_prb"]), d["nof_prb"]), d)
    assert m["p_early"] == 0.0                                   # symbols 0..12: zeros
    assert abs(m["rms"] - 1.0) < TOL                             # unit power per occupied subcarrier
    assert m["leak"] < TOL * m["rms"]                            # off-comb and out-of-band subcarriers
    assert abs(m["h"] - 1.0) < TOL
    others = np.delete(m["corr"], d["n_srs"])
    assert m["corr"][d["n_srs"]] > 1 - TOL and np.all(others < TOL), m["corr"]


def test_planned_resources_match_reference(encoded):
    b, refs, _, _ = encoded
    for i, d in enumerate(refs):
        r, want = b.resource(i), R.resource(**d)
        for f in ("m_srs", "M_sc", "k0", "n_SRS", "T_srs", "u", "v", "nzc", "q", "n_cs"):
            assert getattr(r, f) == int(want[f][0]), (i, f)
        assert list(r.n_b) == want["n_b"][0].tolist(), i


def test_every_sample_written_and_plan_reuse_on_a_side_stream(encoded):
    b, refs, iq, _ = encoded
    side = torch.cuda.Stream()
    a1 = run_batch(b, stream=side, fill=float("nan"))
    assert not np.any(np.isnan(a1))
    a2 = run_batch(b, stream=side, fill=float("nan"))
    assert a1.tobytes() == a2.tobytes() == iq.tobytes()


def test_last_symbol_only_leaves_the_rest_of_the_subframe(encoded):
    b, refs, iq, _ = encoded
    b2 = abi.SrsBatch([product_cfg(d) for d in refs], flags=abi.SRS_FLAG_LAST_SYMBOL_ONLY)
    out = run_batch(b2, fill=7.0)
    for i, d in enumerate(refs):
        got, full, s = piece(b2, out, i, d["nof_prb"]), piece(b, iq, i, d["nof_prb"]), sym13(d["nof_prb"])
        assert np.all(got[:s] == 7.0), i
        assert got[s:].tobytes() == full[s:].tobytes() and not np.any(got[s:] == 7.0), i
    b2.close()


def test_srs_over_a_shortened_pucch(built):
    """a shortened format 1a from mi_pucch_batch_run, then the SRS with MI_SRS_FLAG_LAST_SYMBOL_ONLY on the same
    buffer and stream: both reference receivers still find their signal"""
    for nof_prb, bw_cfg, ack in [(6, 7, 1), (25, 2, 0)]:
        pd = dict(cell_id=58, nof_prb=nof_prb, sf_idx=3, rnti=0x77, fmt=PR.F1A, n_pucch=9, delta=1, N_cs=0, n_rb_2=0, gh=0,
                  shortened=1, cqi_len=0)
        sd = ref_cfg(dict(cell_id=58, nof_prb=nof_prb, bw_cfg=bw_cfg, tti=13, n_srs=5, k_tc=1))
        pb = abi.PucchBatch([abi.pucch_cfg(cell_id=58, nof_prb=nof_prb, sf_idx=3, rnti=0x77, format=abi.PUCCH_1A, n_pucch=9,
                                           shortened=1)])
        sb = abi.SrsBatch([product_cfg(sd)], flags=abi.SRS_FLAG_LAST_SYMBOL_ONLY)
        assert pb.iq_samples == sb.iq_samples
        st = torch.cuda.Stream()
        d_uci = torch.from_numpy(np.array([abi.pucch_uci(ack)], np.uint32).view(np.int32)).cuda()
        d_iq = torch.full((2 * pb.iq_samples,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        pb.run(d_uci.data_ptr(), d_iq.data_ptr(), st.cuda_stream)
        sb.run(d_iq.data_ptr(), st.cuda_stream)
        st.synchronize()
        iq = d_iq.cpu().numpy()
        assert not np.any(np.isnan(iq))
        g = R.demod(iq, nof_prb)
        assert PR.receive(g, pd)[0] == ack
        m = R.receive(g, sd)
        assert m["corr"][5] > 1 - TOL and np.all(np.delete(m["corr"], 5) < TOL) and m["leak"] < TOL
        # the sum of the two reference signals
        want = PR.iq(pd, ack) + R.iq(sd)
        assert rel_err(iq, want) < TOL
        pb.close()
        sb.close()


def test_scale_and_frequency_shift_per_transmission(encoded):
    """d_scale and d_cfo: sample i of subframe k is scale[k] exp(j 2 pi cfo[k] i / N) times the plain one.  The float32
    phase 2 cfo i / N (i < 15 N) is exact to ~1e-6 rad: the batch bound holds."""
    b, refs, _, want = encoded
    rng = np.random.default_rng(11)
    scale = rng.uniform(0.25, 4.0, len(refs)).astype(np.float32)
    cfo = rng.uniform(-0.5, 0.5, len(refs)).astype(np.float32)
    out = run_batch(b, cfo=cfo, scale=scale, fill=float("nan"))
    only_scale = run_batch(b, scale=scale)
    for i, d in enumerate(refs):
        ref = want[i].reshape(-1, 2)
        z = (ref[:, 0] + 1j * ref[:, 1]) * float(scale[i])
        zs = np.stack([z.real, z.imag], 1).astype(np.float32).ravel()
        assert rel_err(piece(b, only_scale, i, d["nof_prb"]), zs) < TOL, i
        z = z * np.exp(2j * np.pi * float(cfo[i]) * np.arange(len(ref)) / R.NFFT[d["nof_prb"]])
        assert rel_err(piece(b, out, i, d["nof_prb"]), np.stack([z.real, z.imag], 1).astype(np.float32).ravel()) < TOL, i


BAD = [dict(cell_id=504), dict(tti=10240), dict(bw_cfg=8), dict(B=4), dict(b_hop=4), dict(n_rrc=24), dict(k_tc=2),
       dict(n_srs=8), dict(I_srs=637), dict(dss=30), dict(nof_prb=7), dict(nof_prb=6, bw_cfg=6), dict(bw_cfg=1)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_batch_create_rejects(built, bad):
    good = ref_cfg(dict(nof_prb=25, bw_cfg=2, B=1))
    assert not R.valid(**dict(good, **bad))
    with pytest.raises(RuntimeError, match="SRS"):
        abi.SrsBatch([product_cfg(good), product_cfg(dict(good, **bad))])


# ---- the per-TTI call --------------------------------------------------------------------------------------
POWER = dict(p0_nominal_pusch=-85.0, alpha=0.7, p0_nominal_pucch=-105.0, delta_f_pucch=(-2.0, 1.0, 2.0, 3.0, -1.0),
             delta_preamble_msg3=4.0, p0_ue_pusch=-3.0, delta_mcs_based=1, acc_enabled=0, p0_ue_pucch=2.0, p_srs_offset=7.0)
PL, P0_PRE = 71.5, -104.0


def run_harness(d, ttis, flags=0, cfo=0.0, configured=1, pusch=0, power=POWER):
    """d: a ref_cfg -> [(ret, srs_power, iq)], powers [9], (pusch rets, before, after)"""
    n = 15 * R.NFFT[d["nof_prb"]]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("20i", d["cell_id"], d["nof_prb"], len(ttis), d["gh"], d["sh"], d["dss"], flags, configured,
                                0, d["bw_cfg"], d["I_srs"], d["B"], d["b_hop"], d["n_rrc"], d["k_tc"], d["n_srs"], pusch,
                                0x46, power["delta_mcs_based"], power["acc_enabled"]))
            f.write(struct.pack("16f", cfo, PL, power["p0_nominal_pusch"], power["alpha"], power["p0_nominal_pucch"],
                                *power["delta_f_pucch"], power["delta_preamble_msg3"], power["p0_ue_pusch"],
                                power["p0_ue_pucch"], power["p_srs_offset"], P0_PRE, 0.0))
            f.write(struct.pack(f"{len(ttis)}i", *ttis))
        subprocess.check_call([HARNESS, fin, fout], timeout=120)
        raw = open(fout, "rb").read()
    out, pos = [], 0
    for _ in ttis:
        ret, = struct.unpack_from("i", raw, pos)
        pw, = struct.unpack_from("f", raw, pos + 4)
        pos += 8
        out.append((ret, pw, np.frombuffer(raw[pos:pos + 8 * n], np.float32)))
        pos += 8 * n
    powers = struct.unpack_from("9f", raw, pos)
    pos += 36
    extra = None
    if pusch:
        pr = struct.unpack_from("2i", raw, pos)
        pos += 8
        extra = (pr, raw[pos:pos + 8 * n], raw[pos + 8 * n:pos + 16 * n])
    return out, powers, extra


HOP = ref_cfg(dict(nof_prb=25, bw_cfg=2, B=1, b_hop=0, n_rrc=4, k_tc=1, n_srs=6, I_srs=9, cell_id=91, gh=1))
# I_SRS = 9: T_SRS = 10, offset 2; N_1 = 6 positions
HOP_TTIS = [2 + 10 * k for k in range(6)]


@pytest.fixture(scope="module")
def per_tti(built):
    assert os.path.exists(HARNESS)
    assert all(abi.lib().srslte_refsignal_srs_send_ue(9, t) == 1 for t in HOP_TTIS)
    return run_harness(HOP, HOP_TTIS, pusch=1)


def test_per_tti_hopping_period_matches_reference(per_tti):
    out, _, _ = per_tti
    k0 = set()
    for (ret, _, iq), tti in zip(out, HOP_TTIS):
        d = dict(HOP, tti=tti)
        assert ret == 0
        assert rel_err(iq, R.iq(d)) < TOL, tti
        b = abi.SrsBatch([product_cfg(d)])
        assert iq.tobytes() == run_batch(b).tobytes()
        b.close()
        k0.add(int(R.resource(**d)["k0"][0]))
    assert len(k0) == 6


def test_per_tti_call_leaves_pusch_and_softbuffer_alone(per_tti):
    """a PUSCH subframe before the SRS calls, and after them from the HARQ softbuffer: byte-identical"""
    (r0, r1), before, after = per_tti[2]
    assert (r0, r1) == (0, 0)
    assert before == after and any(before)


def test_per_tti_power_wrappers_equal_the_host_functions(per_tti):
    out, pw, _ = per_tti
    c = abi.ul_power_cfg(**POWER)
    m_srs = int(R.resource(**HOP)["m_srs"][0])
    # the harness's PUSCH grant: 3 PRB, 256 bits -> one code block of 256 + 24 = 280 bits (a turbo block size)
    assert pw[0] == abi.ul_pusch_power(c, PL, 0.0, 3, 280)
    assert pw[1] == abi.ul_pusch_power(c, PL, P0_PRE, 3, 280) and pw[1] != pw[0]
    for fmt in range(6):
        assert pw[2 + fmt] == abi.ul_pucch_power(c, PL, fmt, 11, 1)
    assert pw[8] == abi.ul_srs_power(c, PL, m_srs) and pw[8] != 0.0
    assert all(p == pw[8] for _, p, _ in out)


def test_per_tti_normalisation_and_cfo(built):
    """set_normalization: nof_prb / (15 sqrt(m_srs / 2)) (the PUSCH factor with L_prb = m_srs / 2); set_cfo:
    exp(j 2 pi cfo n / N) over the subframe's sample index"""
    cfo = -0.41
    d = ref_cfg(dict(nof_prb=50, bw_cfg=0, B=1, n_rrc=13, n_srs=3, cell_id=12, tti=345))
    ((ret, _, iq),), _, _ = run_harness(d, [345], flags=3, cfo=cfo)
    assert ret == 0
    m_srs = int(R.resource(**d)["m_srs"][0])
    assert m_srs == 24
    ref = R.iq(d).reshape(-1, 2)
    z = (ref[:, 0] + 1j * ref[:, 1]) * (50 / 15 / np.sqrt(m_srs / 2))
    z = z * np.exp(2j * np.pi * cfo * np.arange(len(ref)) / R.NFFT[50])
    assert rel_err(iq, np.stack([z.real, z.imag], 1).astype(np.float32).ravel()) < TOL


def test_per_tti_call_rejects(built):
    """SRS not configured, a reserved I_SRS, m_SRS,0 > nof_prb: SRSLTE_ERROR, nothing written, no power"""
    (r, pw, iq), = run_harness(HOP, [2], configured=0)[0]
    assert r == -1 and pw == 0.0 and not np.any(iq)
    (r, _, iq), = run_harness(dict(HOP, I_srs=637), [2])[0]
    assert r == -1 and not np.any(iq)
    (r, pw, iq), = run_harness(dict(HOP, bw_cfg=0), [2])[0]
    assert r == -1 and pw == 0.0 and not np.any(iq)
