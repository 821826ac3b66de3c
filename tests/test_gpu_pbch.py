"""GPU: the PBCH receiver (mi_pbch_*, pbch.hip) against the reference (tests/pbch_ref.py, numpy over oracle
primitives) and transmit-chain ground truth.

Bars: soft bits within 1e-4 relative per port hypothesis (GPU fp32 front end vs the oracle's fp64 one: the bar
and metric of the PDCCH soft bits in test_gpu_ctrl.py); the blind decode on identical soft bits bit-exact
(verdict, port count, 40 ms phase, frames used, bits), also where decoding is marginal and where it needs the
frames combined; a MIB put on the air is read back; bad candidate lists are refused before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import pbch_ref as R
from helpers import rel_err
from srsue_amd import abi

pytestmark = pytest.mark.gpu

H2 = [0.8 + 0.3j, -0.4 + 0.5j]
H2B = [-0.4 + 0.5j, 0.8 + 0.3j]
BW = (6, 15, 25, 50, 75, 100)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert torch.cuda.is_available()


def sf0_cfg(cell_id, nof_prb, ports):
    return abi.sf_cfg(cell_id=cell_id, nof_prb=nof_prb, nof_ports=ports, sf_idx=0, cfi=2, tbs=208, Qm=2)


def tx_frame(cell_id, nof_prb, tx_ports, bits, phase, snr_db, seed, h=H2):
    """subframe 0 of a frame at 40 ms phase `phase` from the product transmitter: CRS + a small PDSCH + the PBCH,
    flat channel h per port, AWGN at snr_db per RE (None = noiseless)"""
    cfg = sf0_cfg(cell_id, nof_prb, tx_ports)
    iq = abi.tx_subframe(cfg, np.zeros(cfg.tbs // 8, np.uint8), h=h[:tx_ports], snr_db=300.0)
    abi.tx_pbch(cell_id, nof_prb, tx_ports, bits, phase, iq, h=h[:tx_ports])
    return R.awgn(iq, snr_db, seed)


def ref_soft_bits(cell_id, nof_prb, rx_ports, iq):
    grid, ce = R.front(cell_id, nof_prb, rx_ports, iq)
    return R.soft_bits(cell_id, nof_prb, rx_ports, grid, ce)


def front_batch(cfgs, iqs):
    b = abi.Batch(cfgs, max_its=1)
    flat = np.zeros(2 * b.iq_samples, np.float32)
    for i, iq in enumerate(iqs):
        o = 2 * b.iq_offset(i)
        flat[o:o + len(iq)] = iq
    d = torch.from_numpy(flat).cuda()
    b.run_stages(3, d.data_ptr(), torch.cuda.current_stream().cuda_stream)   # OFDM + chest
    torch.cuda.synchronize()
    return b, d


# cell ids covering mod 3 = 0, 1, 2; ports 1 and 2; 6, 15 and 50 PRB; noiseless and 5 dB; both channels
PARITY = [(300, 6, 1, None, H2), (301, 6, 2, 5.0, H2), (302, 15, 2, None, H2B), (9, 15, 1, 5.0, H2B),
          (10, 50, 2, 5.0, H2), (11, 50, 1, None, H2B), (499, 6, 2, None, H2B), (500, 50, 2, None, H2)]


def test_soft_bit_parity():
    frames = []
    for i, (cid, nprb, ports, snr, h) in enumerate(PARITY):
        bits = np.random.default_rng(i).integers(0, 2, 24).astype(np.uint8)
        frames.append(tx_frame(cid, nprb, ports, bits, i % 4, snr, 100 + i, h))
    b, d = front_batch([sf0_cfg(c[0], c[1], c[2]) for c in PARITY], frames)
    p = abi.Pbch(b)
    assert p.n_frames == len(PARITY) and [p.frame_of(i) for i in range(len(PARITY))] == list(range(len(PARITY)))
    p.run(torch.cuda.current_stream().cuda_stream, mask=abi.Pbch.LLR)
    got = p.llr()
    for i, (cid, nprb, ports, snr, h) in enumerate(PARITY):
        want = ref_soft_bits(cid, nprb, ports, frames[i])
        for hyp in range(ports):
            e = rel_err(got[i, hyp], want[hyp])
            print(f"frame {i}: cell {cid} prb {nprb} ports {ports} snr {snr} hyp {hyp}: rel_err {e:.3g}")
            assert e < 1e-4, (i, hyp, e)
        if ports == 1:
            assert not got[i, 1].any()
    p.close()
    b.close()


# SNRs (dB per RE) of the decode test, chosen on the CPU with the reference over these very candidates
# (6 PRB, the 2-port front end on 1- and 2-port cells, channel H2).  Reference results there: at LOW (-4 dB) no
# newest frame decodes alone, 13 of 24 candidates are found and 12 of them fail at f = 1 but pass at f = 4; at MID
# (-2 dB) 15 of 24 are found, 9 from one frame; at HIGH (5 dB) all 24 are found from one frame (-5 dB: 7 found,
# -3 dB: 19, 3 dB: 24).  The test asserts the first two properties on the reference's own results.
SNR_LOW, SNR_MID, SNR_HIGH = -4.0, -2.0, 5.0
N_PER_SNR = 24


def decode_candidates():
    """[(snr, cell_id, tx_ports, [(bits, phase)] per frame, soft bits [n][2][480])]: n_frames 1..4, every
    starting phase, candidates that cross a BCH TTI boundary (phase 3 then 0, the next TTI's payload)"""
    out = []
    rng = np.random.default_rng(2024)
    for si, snr in enumerate((SNR_LOW, SNR_MID, SNR_HIGH)):
        for c in range(N_PER_SNR):
            cid = 3 * (7 * c + si) + c % 3
            tx_ports = 1 + c % 2
            # LOW: mostly whole TTIs (start phase 0, 4 frames) so that combining can succeed; else everything
            n = 4 if (snr == SNR_LOW and c % 4 != 3) else 1 + (c // 2) % 4
            ph0 = 0 if (snr == SNR_LOW and c % 4 != 3) else (c // 3) % 4
            sfn8 = int(rng.integers(0, 255))
            frames, soft = [], []
            for i in range(n):
                tti, ph = divmod(ph0 + i, 4)
                bits = R.mib_bits(BW[c % 6], c % 2, c % 4, 4 * (sfn8 + tti))
                iq = tx_frame(cid, 6, tx_ports, bits, ph, snr, 1000 * si + 10 * c + i)
                frames.append((bits, ph))
                soft.append(ref_soft_bits(cid, 6, 2, iq))
            out.append((snr, cid, tx_ports, frames, np.array(soft)))
    return out


def test_decode_bit_exact_on_identical_soft_bits():
    cands = decode_candidates()
    assert len(cands) >= 64
    cfgs, lists = [], []
    for snr, cid, tx_ports, frames, soft in cands:
        lists.append(list(range(len(cfgs), len(cfgs) + len(frames))))
        cfgs += [sf0_cfg(cid, 6, 2)] * len(frames)
    b = abi.Batch(cfgs, max_its=1)
    p = abi.Pbch(b)
    p.set_llr(np.concatenate([c[4] for c in cands]))
    p.set_candidates(lists)
    assert p.n_jobs == sum(len(R.jobs(len(c[3]))) for c in cands)
    p.run(torch.cuda.current_stream().cuda_stream, mask=abi.Pbch.DECODE)
    found = {s: 0 for s in (SNR_LOW, SNR_MID, SNR_HIGH)}
    combined = 0
    for i, (snr, cid, tx_ports, frames, soft) in enumerate(cands):
        want = R.decode(cid, soft)
        got = p.result(i)
        assert (got is None) == (want is None), (i, snr, got, want)
        if got is not None:
            assert got[:3] == want[:3] and np.array_equal(got[3], want[3]), (i, snr, got, want)
            found[snr] += 1
        if snr == SNR_LOW and len(frames) == 4:
            fail1 = not any(R.decode_job(cid, soft, P, f, phi)[0] for P, f, phi in R.jobs(4) if f == 1)
            ok4 = any(R.decode_job(cid, soft, P, f, phi)[0] for P, f, phi in R.jobs(4) if f == 4)
            combined += fail1 and ok4
    print("found per SNR:", found, "combining needed and sufficient at LOW:", combined)
    assert combined >= N_PER_SNR / 4                       # combining is exercised
    assert 0 < found[SNR_MID] < N_PER_SNR                  # mixed verdicts
    p.close()
    b.close()


def test_ground_truth_mib():
    """at SNR_HIGH (every single frame decodes in the reference) the whole GPU path reads the transmitted MIB"""
    class Cell(C.Structure):
        _fields_ = [("nof_prb", C.c_uint32), ("nof_ports", C.c_uint32), ("bw_idx", C.c_uint32), ("id", C.c_uint32),
                    ("cp", C.c_int), ("phich_length", C.c_int), ("phich_resources", C.c_int)]
    cases = [(12, 6, 1, 50, 0, 2, 516), (13, 6, 2, 100, 1, 3, 1023), (14, 15, 2, 6, 0, 0, 1), (15, 50, 1, 25, 1, 1, 770),
             (16, 6, 2, 75, 0, 1, 258), (17, 6, 1, 15, 1, 2, 3)]   # cell, prb, ports; MIB: prb, PHICH length / Ng, SFN
    cfgs, iqs, mibs = [], [], []
    for i, (cid, nprb, ports, mprb, pl, pr, sfn) in enumerate(cases):
        bits = R.mib_bits(mprb, pl, pr, sfn)
        iq = tx_frame(cid, nprb, ports, bits, sfn % 4, SNR_HIGH, 50 + i)
        ref = R.decode(cid, [ref_soft_bits(cid, nprb, 2, iq)])
        assert ref is not None and ref[:3] == (ports, sfn % 4, 1) and np.array_equal(ref[3], bits)
        cfgs.append(sf0_cfg(cid, nprb, 2))
        iqs.append(iq)
        mibs.append(bits)
    b, d = front_batch(cfgs, iqs)
    p = abi.Pbch(b)
    p.set_candidates([[i] for i in range(len(cases))])
    p.run(torch.cuda.current_stream().cuda_stream)
    lib = abi.lib()
    for i, (cid, nprb, ports, mprb, pl, pr, sfn) in enumerate(cases):
        got = p.result(i)
        assert got is not None, i
        assert got[:3] == (ports, sfn % 4, 1) and np.array_equal(got[3], mibs[i]), (i, got)
        cell, osfn = Cell(), C.c_uint32()
        lib.srslte_pbch_mib_unpack(got[3].ctypes.data_as(C.c_void_p), C.byref(cell), C.byref(osfn))
        assert (cell.nof_prb, cell.phich_length, cell.phich_resources, osfn.value + got[1]) == (mprb, pl, pr, sfn)
    p.close()
    b.close()


def test_candidate_validation_before_any_launch():
    cfgs = [sf0_cfg(21, 6, 2), sf0_cfg(21, 6, 2), abi.sf_cfg(cell_id=21, nof_prb=6, nof_ports=2, sf_idx=1, cfi=2, tbs=208, Qm=2),
            sf0_cfg(24, 6, 2)]
    b = abi.Batch(cfgs, max_its=1)
    p = abi.Pbch(b)
    assert p.n_frames == 3 and p.frame_of(2) == -1
    p.set_candidates([[0, 1]])
    assert p.n_jobs == len(R.jobs(2))
    for bad, word in [([[0, 1], [1, 4]], "outside"), ([[0, 2]], "subframe 0"), ([[0, 1], [1, 3]], "different cells"),
                      ([[0, 1, 0, 1, 0]], "1..4"), ([[]], "1..4"), ([[0xFFFFFFFF]], "outside")]:
        with pytest.raises(RuntimeError, match=word):
            p.set_candidates(bad)
        assert p.n_jobs == 0                       # nothing is left to launch
        p.run(torch.cuda.current_stream().cuda_stream, mask=abi.Pbch.DECODE)
        with pytest.raises(RuntimeError):
            p.result(0)
    p.close()
    b.close()
