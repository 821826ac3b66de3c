"""GPU: the PUCCH transmitter (srsue_amd/csrc/pucch.hip through mi_pucch_batch_* and mi_ue_ul_pucch_encode)
against the independent reference of tests/pucch_ref.py: IQ parity for all six formats, the reference receiver
on the product's IQ, orthogonality of the product's own output, every output sample written, plan reuse on a
side stream, the per-TTI call in srsUE's call order (tests/c/ue_pucch_harness.c) and the rejections."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import pucch_ref as R
from srsue_amd import abi

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "ue_pucch_harness")
TOL = 1e-4

# 6 PRB (N = 128) is the smallest size where every index computation runs; the last two cases are 100 PRB
# (N = 2048 and the largest PRB mirror: m = 1 sits at PRB 99 / 0)
CASES = [
    dict(fmt=R.F1, n_pucch=7),
    dict(fmt=R.F1, n_pucch=20, shortened=1),
    dict(fmt=R.F1A, n_pucch=0, ack=0),
    dict(fmt=R.F1A, n_pucch=35, ack=1),
    dict(fmt=R.F1A, n_pucch=40, ack=1, shortened=1),
    dict(fmt=R.F1B, n_pucch=3, delta=2, N_cs=2, ack=0),
    dict(fmt=R.F1B, n_pucch=3, delta=2, N_cs=2, ack=1),
    dict(fmt=R.F1B, n_pucch=3, delta=2, N_cs=2, ack=2),
    dict(fmt=R.F1B, n_pucch=3, delta=2, N_cs=2, ack=3),
    dict(fmt=R.F1B, n_pucch=17, delta=3, N_cs=3, ack=2, shortened=1),
    dict(fmt=R.F1A, n_pucch=1, delta=1, N_cs=4, ack=1),                       # mixed RB (n_pucch < c N_cs / delta)
    dict(fmt=R.F1B, n_pucch=2, delta=2, N_cs=6, n_rb_2=1, ack=3, shortened=1),  # mixed RB
    dict(fmt=R.F2, n_pucch=5, n_rb_2=1, cqi=[1]),
    dict(fmt=R.F2, n_pucch=11, n_rb_2=1, cqi=[1, 0, 1, 1]),
    dict(fmt=R.F2, n_pucch=14, n_rb_2=2, cqi=[0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0]),
    dict(fmt=R.F2A, n_pucch=0, n_rb_2=1, cqi=[0, 0, 1, 0], ack=0),
    dict(fmt=R.F2A, n_pucch=23, n_rb_2=2, cqi=[1] * 11, ack=1),
    dict(fmt=R.F2B, n_pucch=6, n_rb_2=1, cqi=[1, 1, 0, 1], ack=0),
    dict(fmt=R.F2B, n_pucch=6, n_rb_2=1, cqi=[1, 1, 0, 1], ack=1),
    dict(fmt=R.F2B, n_pucch=6, n_rb_2=1, cqi=[1, 1, 0, 1], ack=2),
    dict(fmt=R.F2B, n_pucch=6, n_rb_2=1, cqi=[1, 1, 0, 1], ack=3),
    dict(fmt=R.F2, n_pucch=13, n_rb_2=1, N_cs=3, cqi=[0, 1, 0, 0]),             # format 2 in the mixed RB
    dict(fmt=R.F1A, n_pucch=50, gh=1, ack=1),
    dict(fmt=R.F2B, n_pucch=9, n_rb_2=1, gh=1, cqi=[1, 0, 0, 0, 1, 1, 0], ack=2),
    dict(fmt=R.F1B, n_pucch=41, nof_prb=100, ack=1, shortened=1),
    dict(fmt=R.F2A, n_pucch=13, n_rb_2=3, nof_prb=100, gh=1, cqi=[1, 0, 1, 0, 1], ack=1),
]


def ref_cfg(i, c):
    d = dict(cell_id=150 + 7 * i, nof_prb=6, sf_idx=i % 10, rnti=0x100 + i, delta=1, N_cs=0, n_rb_2=0, gh=0, shortened=0)
    d.update({k: v for k, v in c.items() if k not in ("ack", "cqi")})
    d["cqi_len"] = len(c.get("cqi", ()))
    return d


def product_cfg(d):
    return abi.pucch_cfg(cell_id=d["cell_id"], nof_prb=d["nof_prb"], sf_idx=d["sf_idx"], rnti=d["rnti"], format=d["fmt"],
                         n_pucch=d["n_pucch"], delta_shift=d["delta"], N_cs=d["N_cs"], n_rb_2=d["n_rb_2"],
                         group_hopping=d["gh"], shortened=d["shortened"], cqi_len=d["cqi_len"])


def rel_err(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def run_batch(b, words, stream=None, fill=0.0):
    d_uci = torch.from_numpy(np.asarray(words, np.uint32).view(np.int32)).cuda()
    d_iq = torch.full((2 * b.iq_samples,), fill, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = stream or torch.cuda.current_stream()
    b.run(d_uci.data_ptr(), d_iq.data_ptr(), s.cuda_stream)
    s.synchronize()
    return d_iq.cpu().numpy()


def piece(b, iq, i, nof_prb):
    o = 2 * b.iq_offset(i)
    return iq[o:o + 2 * 15 * R.NFFT[nof_prb]]


@pytest.fixture(scope="module")
def encoded(built):
    refs = [ref_cfg(i, c) for i, c in enumerate(CASES)]
    b = abi.PucchBatch([product_cfg(d) for d in refs])
    words = [abi.pucch_uci(c.get("ack", 0), c.get("cqi", ())) for c in CASES]
    iq = run_batch(b, words)
    want = [R.iq(d, c.get("ack", 0), c.get("cqi", ())) for d, c in zip(refs, CASES)]
    return b, refs, iq, want


@pytest.mark.parametrize("i", range(len(CASES)))
def test_batch_iq_matches_reference(encoded, i):
    b, refs, iq, want = encoded
    got = piece(b, iq, i, refs[i]["nof_prb"])
    e = rel_err(got, want[i])
    print("rel_err", i, e)
    assert e < TOL


@pytest.mark.parametrize("i", range(len(CASES)))
def test_reference_receiver_recovers_the_bits(encoded, i):
    b, refs, iq, _ = encoded
    d, c = refs[i], CASES[i]
    ack, cqi = R.receive(R.demod(piece(b, iq, i, d["nof_prb"]), d["nof_prb"]), d)
    two = d["fmt"] in (R.F1B, R.F2B)
    want_ack = 0 if d["fmt"] in (R.F1, R.F2) else c.get("ack", 0) & (3 if two else 1)
    assert ack == want_ack and cqi == list(c.get("cqi", []))


def test_planned_resources_match_reference(encoded):
    b, refs, _, _ = encoded
    for i, d in enumerate(refs):
        r, want = b.resource(i), R.resource(**d)
        assert list(r.n_prb) == want["n_prb"][0].tolist() and list(r.u) == want["u"].tolist()
        assert list(r.n_prime) == want["n_prime"][0].tolist() and list(r.n_oc) == want["n_oc"][0].tolist()
        assert [list(x) for x in r.n_cs] == want["n_cs"][0].tolist()


def test_all_thirty_sequence_groups(built):
    """the kernel's own copy of the M_sc = 12 base sequences, every group u, against the oracle's"""
    refs = [dict(ref_cfg(0, dict(fmt=R.F1A, n_pucch=4)), cell_id=u) for u in range(30)]
    b = abi.PucchBatch([product_cfg(d) for d in refs])
    iq = run_batch(b, [1] * 30)
    for i, d in enumerate(refs):
        assert rel_err(piece(b, iq, i, 6), R.iq(d, 1)) < TOL, i


def test_product_output_is_orthogonal_on_one_prb(built):
    """resources of one PRB, different n': after the reference demodulator the slot inner products of the product's
    own transmissions vanish (data and DMRS symbols separately)"""
    base = dict(fmt=R.F1B, delta=2, N_cs=0)
    ns = [0, 1, 5, 6, 11, 17]          # all m = 0: n' = 0..17 covers every n_oc and several cyclic shifts
    refs = [dict(ref_cfg(3, dict(base, n_pucch=n)), cell_id=33) for n in ns]
    b = abi.PucchBatch([product_cfg(d) for d in refs])
    iq = run_batch(b, [abi.pucch_uci(i % 4) for i in range(len(ns))])
    vec = [R.slot_vectors(R.demod(piece(b, iq, i, 6), 6), d) for i, d in enumerate(refs)]
    for s in range(2):
        for part in range(2):
            V = np.stack([v[s][part] for v in vec])
            G = np.abs(V @ V.conj().T)
            energy = np.diag(G).copy()
            np.fill_diagonal(G, 0)
            assert G.max() < 1e-4 * energy.min(), (s, part, G.max(), energy.min())


def test_every_sample_written_and_plan_reuse_on_a_side_stream(encoded):
    b, refs, _, _ = encoded
    words = [abi.pucch_uci(c.get("ack", 0), c.get("cqi", ())) for c in CASES]
    iq = run_batch(b, words, fill=7.0)
    assert not np.any(iq == 7.0)
    for i, d in enumerate(refs):
        N = R.NFFT[d["nof_prb"]]
        last = piece(b, iq, i, d["nof_prb"])[2 * (15 * N - N - 144 * N // 2048):]
        assert np.all(last == 0.0) == bool(d["shortened"]), i
    # other UCI words, the same plan, a side stream
    rng = np.random.default_rng(5)
    acks = rng.integers(0, 4, len(CASES))
    cqis = [rng.integers(0, 2, d["cqi_len"]).tolist() for d in refs]
    iq2 = run_batch(b, [abi.pucch_uci(int(a), q) for a, q in zip(acks, cqis)], stream=torch.cuda.Stream(), fill=7.0)
    assert not np.any(iq2 == 7.0)
    for i, d in enumerate(refs):
        assert rel_err(piece(b, iq2, i, d["nof_prb"]), R.iq(d, int(acks[i]), cqis[i])) < TOL, i


BAD = [dict(delta=0), dict(delta=4), dict(N_cs=8), dict(delta=2, N_cs=3), dict(n_pucch=216),
       dict(fmt=R.F2, cqi=[1, 0], shortened=1), dict(fmt=R.F2), dict(fmt=R.F2A, cqi=[0] * 12), dict(nof_prb=7)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_batch_create_rejects(built, bad):
    good = ref_cfg(0, dict(fmt=R.F1A, n_pucch=4))
    with pytest.raises(RuntimeError, match="PUCCH"):
        abi.PucchBatch([product_cfg(good), product_cfg(ref_cfg(1, dict(dict(fmt=R.F1A, n_pucch=4), **bad)))])


# ---- the per-TTI call --------------------------------------------------------------------------------------
def run_harness(cell_id, nof_prb, calls, gh=0, flags=0, cfo=0.0, delta=1, N_cs=0, n_rb_2=1, srs=(0, 0, 0),
                sched=(11, 3, 29), rnti=0x46, pusch=0):
    """calls: dict(tti, n_cce, ack_len, ack, sr, cqi) -> [((ret, format, shortened), iq)], (pusch rets, before, after)"""
    n = 15 * R.NFFT[nof_prb]
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("16i", cell_id, nof_prb, len(calls), gh, flags, delta, N_cs, n_rb_2, *srs, *sched, rnti,
                                pusch))
            f.write(struct.pack("f", cfo))
            for c in calls:
                cqi = list(c.get("cqi", ()))
                f.write(struct.pack("6i", c["tti"], c.get("n_cce", 0), c.get("ack_len", 0), c.get("ack", 0),
                                    int(c.get("sr", 0)), len(cqi)))
                f.write(bytes(cqi + [0] * (64 - len(cqi))))
        subprocess.check_call([HARNESS, fin, fout], timeout=120)
        raw = open(fout, "rb").read()
    out, pos = [], 0
    for _ in calls:
        r = struct.unpack_from("3i", raw, pos)
        pos += 12
        out.append((r, np.frombuffer(raw[pos:pos + 8 * n], np.float32)))
        pos += 8 * n
    extra = None
    if pusch:
        pr = struct.unpack_from("2i", raw, pos)
        pos += 8
        extra = (pr, raw[pos:pos + 8 * n], raw[pos + 8 * n:pos + 16 * n])
    return out, extra


def one_entry_batch(d, ack, cqi):
    b = abi.PucchBatch([product_cfg(d)])
    return run_batch(b, [abi.pucch_uci(ack, cqi)])


# (call, selected format, selected resource) for N_pucch_1 = 11, n_pucch_2 = 3, n_pucch_sr = 29
Q = [1, 0, 1, 1]
ROWS = [(dict(tti=14, n_cce=7, ack_len=1, ack=1), R.F1A, 18),
        (dict(tti=25, n_cce=2, ack_len=2, ack=2), R.F1B, 13),
        (dict(tti=36, n_cce=7, ack_len=1, ack=0, sr=1), R.F1A, 29),
        (dict(tti=47, n_cce=7, ack_len=2, ack=3, sr=1), R.F1B, 29),
        (dict(tti=58, sr=1), R.F1, 29),
        (dict(tti=69, cqi=Q), R.F2, 3),
        (dict(tti=70, n_cce=7, cqi=Q, ack_len=1, ack=1), R.F2A, 3),
        (dict(tti=81, n_cce=7, cqi=Q, ack_len=2, ack=1), R.F2B, 3),
        (dict(tti=92, cqi=Q, sr=1), R.F1, 29)]


@pytest.fixture(scope="module")
def per_tti(built):
    assert os.path.exists(HARNESS)
    return run_harness(91, 6, [r[0] for r in ROWS], gh=1, pusch=1)


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_per_tti_call_selects_and_encodes(per_tti, i):
    call, fmt, n_pucch = ROWS[i]
    (ret, last_format, shortened), iq = per_tti[0][i]
    assert (ret, last_format, shortened) == (0, fmt, 0)
    cqi = call.get("cqi", []) if fmt >= R.F2 else []
    d = dict(cell_id=91, nof_prb=6, sf_idx=call["tti"] % 10, rnti=0x46, fmt=fmt, n_pucch=n_pucch, delta=1, N_cs=0,
             n_rb_2=1, gh=1, shortened=0, cqi_len=len(cqi))
    assert np.array_equal(iq, one_entry_batch(d, call.get("ack", 0), cqi))
    assert rel_err(iq, R.iq(d, call.get("ack", 0), cqi)) < TOL


def test_per_tti_call_leaves_pusch_and_softbuffer_alone(per_tti):
    """a PUSCH subframe before the PUCCH calls, and after them from the HARQ softbuffer: byte-identical"""
    (r0, r1), before, after = per_tti[1]
    assert (r0, r1) == (0, 0)
    assert before == after and any(before)


def test_per_tti_shortened_in_srs_subframes(built):
    """srs_cs_subf_cfg 7: cell-specific SRS in subframes 0 and 1 of every 5"""
    ack = dict(n_cce=4, ack_len=1, ack=1)
    calls = [dict(tti=11, **ack), dict(tti=12, **ack), dict(tti=16, cqi=Q)]
    on, _ = run_harness(5, 6, calls, srs=(1, 7, 1))
    assert [r[0] for r in on] == [(0, R.F1A, 1), (0, R.F1A, 0), (0, R.F2, 0)]
    d = dict(cell_id=5, nof_prb=6, sf_idx=1, rnti=0x46, fmt=R.F1A, n_pucch=15, delta=1, N_cs=0, n_rb_2=1, gh=0,
             shortened=1, cqi_len=0)
    assert rel_err(on[0][1], R.iq(d, 1)) < TOL
    off, _ = run_harness(5, 6, calls[:1], srs=(1, 7, 0))        # srs_simul_ack off
    assert off[0][0] == (0, R.F1A, 0)
    assert rel_err(off[0][1], R.iq(dict(d, shortened=0), 1)) < TOL
    none, _ = run_harness(5, 6, calls[:1], srs=(0, 7, 1))       # no SRS configured
    assert none[0][0] == (0, R.F1A, 0)


def test_per_tti_normalisation_and_cfo(built):
    """set_normalization: nof_prb / 15 (the PUSCH factor with L_prb = 1); set_cfo: exp(j 2 pi cfo n / N) over the
    subframe's sample index.  The float32 phase 2 cfo n / N (n < 15 N) is exact to ~1e-6 rad: the batch bound holds."""
    cfo = 0.37
    (r, iq), = run_harness(3, 25, [dict(tti=5, n_cce=9, ack_len=2, ack=2)], flags=3, cfo=cfo, n_rb_2=0)[0]
    assert r == (0, R.F1B, 0)
    d = dict(cell_id=3, nof_prb=25, sf_idx=5, rnti=0x46, fmt=R.F1B, n_pucch=20, delta=1, N_cs=0, n_rb_2=0, gh=0,
             shortened=0, cqi_len=0)
    ref = R.iq(d, 2).reshape(-1, 2)
    z = (ref[:, 0] + 1j * ref[:, 1]) * (25 / 15) * np.exp(2j * np.pi * cfo * np.arange(len(ref)) / R.NFFT[25])
    assert rel_err(iq, np.stack([z.real, z.imag], 1).astype(np.float32).ravel()) < TOL


def test_per_tti_call_rejects(built):
    """an invalid PUCCH configuration, a CQI too long for format 2, no UCI at all: an error, nothing written"""
    ack = dict(tti=3, n_cce=1, ack_len=1, ack=1)
    for kw, call in [(dict(delta=0), ack), (dict(delta=2, N_cs=3), ack), (dict(sched=(300, 3, 29)), ack),
                     (dict(), dict(tti=3, cqi=[1] * 12)), (dict(), dict(tti=3))]:
        (r, iq), = run_harness(9, 6, [call], **kw)[0]
        assert r[0] != 0 and r[1] == 99 and not np.any(iq), (kw, call)
