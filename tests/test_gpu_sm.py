"""GPU: two-layer spatial multiplexing (tm 3 / 4) of the batched receiver against tests/pdsch_sm_ref.py.

A spatially multiplexed subframe is a cw 0 / cw 1 pair of cfg entries on a two-antenna batch.  Float stages at the
project's 1e-4 through helpers.rel_err, decoder outputs exact.

(a) detection alone against the reference  (b) end to end  (c) HARQ on codeword 1  (d) group shapes  (e) API edges."""
import ctypes as C

import numpy as np
import pytest
import torch

import pdsch_ref as R
import pdsch_ref_util as U
import pdsch_rx_ref as X
import pdsch_sm_ref as S
from helpers import rel_err
from srsue_amd import abi
from test_gpu_pdsch_ref import TOL, demap_cfgs, ri, stream
from test_gpu_rx_div import iq_planes, plane_buffer, plane_part

pytestmark = pytest.mark.gpu

S_OFDM, S_CHEST, S_DEMAP, S_RM, S_TDEC, S_TB = (1 << i for i in range(6))


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert torch.cuda.is_available()


def twice(per_pair):
    """per-entry list of a batch of pairs only: each pair's item for its cw 0 and its cw 1 entry (one offset)"""
    return [x for x in per_pair for _ in range(2)]


def emu_decode_its(cfgs, llrs, i16, max_its=4):
    """emu_decode_llr (lane schedule): payload bytes, TB CRC and TB iteration counts per entry"""
    arr = abi.cfg_array(cfgs)
    flat = np.ascontiguousarray(np.concatenate(llrs), np.float32)
    pay = np.zeros(sum(c.tbs // 8 for c in cfgs), np.uint8)
    ok, its = np.zeros(len(cfgs), np.uint32), np.zeros(len(cfgs), np.uint32)
    E = abi.emu()
    E.emu_set_tdec_i16(int(i16))
    try:
        assert E.emu_decode_llr(C.cast(arr, C.c_void_p), len(cfgs), flat.ctypes.data, max_its, pay.ctypes.data,
                                ok.ctypes.data, its.ctypes.data, None) == 0
    finally:
        E.emu_set_tdec_i16(0)
    return pay, ok, its


def entry_llrs(b, cfgs, llr):
    """the downloaded LLR stream cut into the entries' G values"""
    return [llr[b.offset(abi.BUF_LLR, i):b.offset(abi.BUF_LLR, i) + abi.pdsch_G(c)] for i, c in enumerate(cfgs)]


# ------------------------------------------------------------------------------------------------ (a) detection alone
def test_detection_against_reference():
    """DEMAP alone on uploaded reference grids and estimates: one two-antenna batch of the nine pairs of the CPU test
    (all Qm combinations of the table, the three precoders, 6 .. 100 PRB, a distributed allocation) with a TM1 and a
    TM2 entry between them.  Every codeword's stream == the reference at 1e-4; the TM1 / TM2 entries == pdsch_llr_rx."""
    pairs = S.detect_pairs()
    ins, _ = S.detect_inputs()
    others = (demap_cfgs()[4], demap_cfgs()[3])              # Qm 6 TM1, Qm 4 TM2 (15 PRB)
    oins = X.demap_rx_inputs(others)
    entries = []                                             # (kind, object, grids, ces, codeword)
    for j, (p, (g, h)) in enumerate(zip(pairs, ins)):
        if j in (4, 7):
            k = 0 if j == 4 else 1
            entries.append(("rx", others[k], oins[k][0], oins[k][1], 0))
        entries += [("sm", p, g, h, 0), ("sm", p, g, h, 1)]
    cfgs = [U.to_abi(o) if kind == "rx" else o.abi()[q] for kind, o, _, _, q in entries]
    b = abi.Batch(cfgs, n_rx=2)
    b.upload(abi.BUF_GRID, plane_buffer(b, abi.BUF_GRID, [[e[2][a] for e in entries] for a in range(2)]))
    b.upload(abi.BUF_CE, plane_buffer(b, abi.BUF_CE, [[e[3][a] for e in entries] for a in range(2)]))
    b.run_stages(S_DEMAP, None, stream())
    got = entry_llrs(b, cfgs, b.download(abi.BUF_LLR, np.float32))
    worst = dict(sm=0.0, rx=0.0)
    want_sm = {}
    for i, (kind, o, g, h, q) in enumerate(entries):
        if kind == "rx":
            want = X.pdsch_llr_rx(o, X.as_grids(o, g), X.as_ces(o, h))
        else:
            if id(o) not in want_sm:
                want_sm[id(o)] = S.pdsch_llr_sm(o, S.as_grids(o, g), S.as_ces(o, h))
            want = want_sm[id(o)][q]
        assert len(got[i]) == len(want)
        e = rel_err(got[i], want)
        worst[kind] = max(worst[kind], e)
        assert e < TOL, (i, kind, q, e)
    print(f"(a) detection: worst llr rel_err sm {worst['sm']:.3e}, tm1 / tm2 {worst['rx']:.3e}")
    b.close()


# ------------------------------------------------------------------------------------------------ (b) end to end
def e2e_batch_inputs():
    cases = [S.e2e_samples(seed, prec, S.E2E_MCS[0]) for seed in (0, 1, 2) for prec in S.PRECODERS]
    cfgs = [c for p, _, _ in cases for c in p.abi()]
    tbs = [t for _, ts, _ in cases for t in ts]
    iqs = [twice([U.f32c(s[a]) for _, _, s in cases]) for a in range(2)]
    return cases, cfgs, tbs, iqs


@pytest.mark.parametrize("i16", [True, False], ids=["i16", "gen"])
def test_end_to_end(i16):
    """The whole chain on the reference's samples (6 PRB, 30 dB, a selective channel per antenna; seeds 0..2 x the
    three precoders, 16QAM / 64QAM): grid and ce planes == the reference front end, both payloads == the transmitted
    ones with tb_crc 1, and payload, CRC and iteration counts == emu_decode_llr on the downloaded LLR stream."""
    cases, cfgs, tbs, iqs = e2e_batch_inputs()
    b = abi.Batch(cfgs, max_its=4, tdec_i16=i16, n_rx=2)
    assert b.iq_samples == len(cases) * 15 * 128
    b.run(iq_planes(b, iqs).data_ptr(), stream())
    torch.cuda.synchronize()
    grid, ce, llr = (b.download(k, np.float32) for k in (abi.BUF_GRID, abi.BUF_CE, abi.BUF_LLR))
    pay, crc, its = b.download(abi.BUF_PAYLOAD, np.uint8), b.download(abi.BUF_TB_CRC, np.uint32), \
        b.download(abi.BUF_TB_ITS, np.uint32)
    worst = dict(grid=0.0, ce=0.0)
    for j, (p, _, _) in enumerate(cases):
        rg, rc = S.front(p, [U.c128(iqs[a][2 * j]) for a in range(2)])
        for a in range(2):
            eg = rel_err(plane_part(b, abi.BUF_GRID, grid, a, 2 * j, 2 * rg[a].size), ri(rg[a]))
            ec = rel_err(plane_part(b, abi.BUF_CE, ce, a, 2 * j + 1, 2 * rc[a].size), ri(rc[a]))   # cw 1: the partner's offset
            worst = dict(grid=max(worst["grid"], eg), ce=max(worst["ce"], ec))
            assert eg < TOL and ec < TOL, (j, a, eg, ec)
    for i in range(len(cfgs)):
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs[i]), i
    epay, eok, eits = emu_decode_its(cfgs, entry_llrs(b, cfgs, llr), i16)
    assert np.array_equal(pay, epay) and np.array_equal(crc, eok) and np.array_equal(its, eits)
    print("(b) end to end: worst rel_err " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    b.close()


# ------------------------------------------------------------------------------------------------ (c) HARQ
def test_harq_on_codeword_1():
    """Codeword 1 at rv 0, then at rv 2 with new_tb = 0 through a re-plan, codeword 0 a new transport block both times,
    at the SNR test_pdsch_sm_ref.py pins (codeword 1 fails alone, passes combined).  CRCs as pinned; the payloads and the
    final softbuffer == the emulated chain fed each transmission's LLR stream."""
    tx = S.harq_samples()
    b = abi.Batch(tx[0][0].abi(), max_its=4, n_rx=2)
    plan = abi.Plan()
    E = abi.emu()
    E.emu_keep_softbuffer(1)
    try:
        for t, (p, tbs, iqs) in enumerate(tx):
            cfgs = p.abi(new_tb=(1, int(t == 0)))
            if t:
                plan.build(cfgs)
                b.replan(plan, stream())
            b.run(iq_planes(b, [twice([U.f32c(iqs[a])]) for a in range(2)]).data_ptr(), stream())
            torch.cuda.synchronize()
            crc = b.download(abi.BUF_TB_CRC, np.uint32)
            assert crc.tolist() == [1, int(t == 1)], (t, crc.tolist())
            pay = b.download(abi.BUF_PAYLOAD, np.uint8)
            epay, eok, _ = emu_decode_its(cfgs, entry_llrs(b, cfgs, b.download(abi.BUF_LLR, np.float32)), True)
            assert np.array_equal(pay, epay) and np.array_equal(crc, eok), t
        for q in range(2):
            assert np.array_equal(b.payload(q, pay), tbs[q]), q
        sb = b.download(abi.BUF_SB, np.float32)
        esb = np.zeros(E.emu_softbuffer(None), np.float32)
        E.emu_softbuffer(esb.ctypes.data)
        assert len(esb) == len(sb) and esb.any() and np.array_equal(sb, esb), int((sb != esb).sum())
    finally:
        E.emu_keep_softbuffer(0)
    plan.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (d) group shapes
FLAT_H = ((0.9, 0.3 + 0.2j), (-0.2 + 0.3j, 0.8))          # [antenna][port]


def test_group_shapes():
    """70 pairs of 6 PRB (140 transport blocks: per code-block size a full and a partial 64-lane group) and one 100-PRB
    pair (64QAM / 64QAM, tbs 36696 each, six code blocks per codeword) from the product's transmitter through a flat
    2 x 2 channel with |det| >= 0.3 at 30 dB, in one batch: every payload exact."""
    assert abs(np.linalg.det(np.array(FLAT_H))) >= 0.3
    pairs = [S.Pair((3, 4, 4)[i % 3], (0, 1, 2)[i % 3], (4, 6), (1000, 1544), cell_id=50 + i % 5, nof_prb=6, sf=1 + i % 4, cfi=1,
                    rnti=0x400 + i) for i in range(70)]
    pairs.append(S.Pair(3, 0, (6, 6), (36696, 36696), cell_id=77, nof_prb=100, sf=1, cfi=1, rnti=0x500))
    tbs = [[U.tb_bytes(2000 + 2 * i + q, p.cw[q].tbs) for q in range(2)] for i, p in enumerate(pairs)]
    iqs = [twice([abi.tx_subframe_sm(p.abi(), t[0], t[1], h=list(FLAT_H[a]), snr_db=30.0, seed=9000 + 2 * i + a)
                  for i, (p, t) in enumerate(zip(pairs, tbs))]) for a in range(2)]
    cfgs = [c for p in pairs for c in p.abi()]
    b = abi.Batch(cfgs, max_its=4, n_rx=2)
    assert b.n_codeblocks == 140 + 12 and b.n_groups == 2 * 2 + 1
    b.run(iq_planes(b, iqs).data_ptr(), stream())
    torch.cuda.synchronize()
    pay, crc = b.download(abi.BUF_PAYLOAD, np.uint8), b.download(abi.BUF_TB_CRC, np.uint32)
    for i, t in enumerate(tbs):
        for q in range(2):
            assert crc[2 * i + q] == 1 and np.array_equal(b.payload(2 * i + q, pay), t[q]), (i, q)
    b.close()


# ------------------------------------------------------------------------------------------------ (e) edges
def test_one_antenna_is_refused():
    pair = S.e2e_pair(0, (4, 1), S.E2E_MCS[0]).abi()
    with pytest.raises(RuntimeError, match="needs n_rx = 2"):
        abi.Batch(pair)
    with pytest.raises(RuntimeError, match="needs n_rx = 2"):
        abi.Pipe(pair)
    b = abi.Batch([abi.sf_cfg(nof_prb=6, tbs=104, Qm=2)])
    plan = abi.Plan().build(pair)
    with pytest.raises(RuntimeError, match="needs n_rx = 2"):
        b.replan(plan, stream())
    plan.close()
    b.close()


def test_stage_runs_offsets_and_pipe():
    """run_stages(DEMAP | RM | TDEC | TB) without keep_llr on uploaded reference grids and estimates decodes (the path
    is forced unfused, also with compact estimates asked for); a cw = 1 entry's offsets are its partner's; the host-IQ
    pipeline accepts a plan with pairs."""
    p, tbs, iqs = S.e2e_samples(1, (4, 2), S.E2E_MCS[2])
    tm1 = abi.sf_cfg(cell_id=3, nof_prb=6, nof_ports=1, sf_idx=2, cfi=1, tbs=1000, Qm=4)
    tb1 = U.tb_bytes(77, tm1.tbs)
    iq1 = [abi.tx_subframe(tm1, tb1, h=[FLAT_H[a][0]], snr_db=30.0, seed=40 + a) for a in range(2)]
    cfgs = [tm1] + p.abi()
    all_iqs = [[iq1[a]] + twice([U.f32c(iqs[a])]) for a in range(2)]
    want = [tb1] + tbs
    b = abi.Batch(cfgs, max_its=4, n_rx=2, compact_ce=True)
    for which in (abi.BUF_GRID, abi.BUF_CE, abi.BUF_METRICS):
        assert b.offset(which, 1) != b.offset(which, 0)
    for which in (abi.BUF_GRID, abi.BUF_CE):
        assert b.offset(which, 2) == b.offset(which, 1)
    assert b.iq_offset(2) == b.iq_offset(1) == 15 * 128 and b.iq_samples == 2 * 15 * 128
    assert b.offset(abi.BUF_LLR, 2) > b.offset(abi.BUF_LLR, 1) and b.offset(abi.BUF_PAYLOAD, 2) == (1000 + 1544) // 8
    d = iq_planes(b, all_iqs)
    b.upload(abi.BUF_METRICS, np.zeros(2 * 3 * 5, np.float32))
    b.run_stages(S_OFDM | S_CHEST, d.data_ptr(), stream())
    b.run_stages(S_DEMAP | S_RM | S_TDEC | S_TB, None, stream())          # after a full-estimate CHEST: not refused
    torch.cuda.synchronize()
    pay, crc = b.download(abi.BUF_PAYLOAD, np.uint8), b.download(abi.BUF_TB_CRC, np.uint32)
    for i in range(3):
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), want[i]), i
    met = b.download(abi.BUF_METRICS, np.float32).reshape(2, 3, 5)
    assert (met[:, :2] > 0).all() and not met[:, 2].any()                 # the cw = 1 row is never written
    host_iq = d.cpu().numpy()
    b.close()
    pipe = abi.Pipe(cfgs, max_its=4, n_rx=2)
    hb = abi.HostBuffer(host_iq.nbytes)
    hb.array[:] = host_iq
    slot = pipe.submit(hb.ptr)
    pipe.wait(slot)
    pb = pipe.batch(slot)
    pay, crc = pb.download(abi.BUF_PAYLOAD, np.uint8), pb.download(abi.BUF_TB_CRC, np.uint32)
    for i in range(3):
        assert crc[i] == 1 and np.array_equal(pb.payload(i, pay), want[i]), i
    pipe.close()
    hb.close()
