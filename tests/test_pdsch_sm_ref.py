"""CPU: two-layer spatial multiplexing (TM3 / TM4).  The float64 reference (tests/pdsch_sm_ref.py) against the spec's
closed forms, the kernel's arithmetic (sm_body.h through the host emulation's emu_pdsch_llr_sm) and the product's
transmitter against that reference, the reference chain end to end, and the emulated chain on the same samples."""
import ctypes as C
import functools

import numpy as np
import pytest

import pdsch_ref as R
import pdsch_ref_util as U
import pdsch_sm_ref as S
from helpers import rel_err
from srsue_amd import abi
from test_pdsch_ref import emu_decode

TOL = 1e-4          # the project's float tolerance (BASELINE.json north_star) through helpers.rel_err


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


# ------------------------------------------------------------------------------------------------ 1: precoder identities
def test_precoder_identities():
    i = np.arange(64)
    for tm, pmi in S.PRECODERS:
        P = S.precoder(tm, pmi, i)
        assert np.allclose(P, S.precoder_closed(tm, pmi, i), atol=1e-15), (tm, pmi)
        assert np.allclose(np.conj(np.swapaxes(P, 1, 2)) @ P, np.eye(2) / 2, atol=1e-15), (tm, pmi)
    P3 = S.precoder(3, 0, i)
    assert np.allclose(P3[2:], P3[:-2], atol=1e-15) and not np.allclose(P3[1], P3[0])      # period 2, not 1
    assert np.allclose(S.precoder(4, 1, i), S.CODEBOOK_2L[1]) and np.allclose(S.precoder(4, 2, i), S.CODEBOOK_2L[2])


def test_layer_index_is_not_the_subcarrier_parity():
    """inside a CRS symbol the running RE index i and the subcarrier index k differ in parity: a detector that takes
    (-1)^k for TM3's (-1)^i is wrong there"""
    p = S.Pair(3, 0, (2, 2), (104, 104), cell_id=30, nof_prb=6, sf=1, cfi=1)
    mask = p.re_mask()
    l, k = np.nonzero(mask)
    i = np.arange(len(k))
    differs = (i % 2) != (k % 2)
    assert differs.any() and not differs.all()
    crs_rows = [r for r in (4, 7, 11) if mask[r].any()]
    for r in crs_rows:           # two of every three subcarriers carry PDSCH: the parity of i - k flips along the row
        d = ((i - k) % 2)[l == r]
        assert d.min() == 0 and d.max() == 1, r


# ------------------------------------------------------------------------------------------------ 2: the kernel arithmetic
def emu_llr_sm(pair, g32s, c32s, noise=0.01):
    arr = abi.cfg_array(pair.abi())
    out = [np.zeros(pair.nre * c.Qm, np.float32) for c in pair.cw]
    g = np.ascontiguousarray(np.concatenate(g32s), np.float32)
    h = np.ascontiguousarray(np.concatenate(c32s), np.float32)
    n = abi.emu().emu_pdsch_llr_sm(C.cast(arr, C.c_void_p), g.ctypes.data, h.ctypes.data, noise, out[0].ctypes.data,
                                   out[1].ctypes.data)
    assert n == pair.nre, n
    return out


def test_emulated_detector_matches_reference():
    """sm_body.h's detection (closed 2 x 2 MMSE in float32, demapper, per-codeword descrambling), compiled for the
    host, == the reference's np.linalg.solve chain at 1e-4 for both codewords of the eight table configurations and
    the distributed allocation; the inputs keep det(G^H G + 0.01 I) >= 5e-3"""
    pairs = S.detect_pairs()
    ins, lowest = S.detect_inputs()
    worst = 0.0
    for j, (p, (g32s, c32s)) in enumerate(zip(pairs, ins)):
        got = emu_llr_sm(p, g32s, c32s)
        want = S.pdsch_llr_sm(p, S.as_grids(p, g32s), S.as_ces(p, c32s))
        for q in range(2):
            e = rel_err(got[q], want[q])
            worst = max(worst, e)
            assert e < TOL, (j, q, p.c.nof_prb, p.tm, p.pmi, e)
    print(f"emulated sm llr: worst rel_err {worst:.3e}, lowest det {lowest:.3e}")


# ------------------------------------------------------------------------------------------------ 3: the transmitter
TX_SM_CASES = [
    dict(tm=3, pmi=0, Qm=(2, 6), tbs=(208, 1544), cell_id=301, nof_prb=6, sf=0, cfi=1),
    dict(tm=4, pmi=1, Qm=(4, 4), tbs=(2856, 2088), cell_id=7, nof_prb=15, sf=5, cfi=2, rnti=0x1234, rv=(2, 0)),
    dict(tm=4, pmi=2, Qm=(6, 2), tbs=(7000, 1000), cell_id=11, nof_prb=25, sf=4, cfi=3, rv=(0, 3)),
    dict(tm=3, pmi=0, Qm=(6, 6), tbs=(36696, 36696), cell_id=503, nof_prb=100, sf=3, cfi=2, rv=(1, 1)),
]


@pytest.mark.parametrize("case", range(len(TX_SM_CASES)))
def test_transmitter_equals_reference_iq(case):
    """Noiseless mi_tx_subframe_sm == the reference's two-codeword grids through a flat h per antenna, to float32
    rounding (the bound test_pdsch_ref.py applies to the one-codeword transmitters): per-codeword coding and scrambling,
    layer mapping, the precoder's index i, CRS, PCFICH, OFDM"""
    pair = S.Pair(**TX_SM_CASES[case])
    tbs = [U.tb_bytes(60 + 2 * case + q, pair.cw[q].tbs) for q in range(2)]
    grids = S.tx_grid(pair, tbs)
    for a, h in enumerate(([0.75 + 0.25j, -0.5 + 0.625j], [0.3 - 0.8j, 0.9 + 0.1j])):
        H = np.array(h)[:, None, None] * np.ones((2, R.NSYMB, pair.c.W))
        want = U.f32c(R.ofdm_tx(grids, H)).astype(np.float64)
        bound = 2 * 2.0 ** -23 * np.max(np.abs(want))
        iq = abi.tx_subframe_sm(pair.abi(), tbs[0], tbs[1], h=h, snr_db=300.0)
        err = np.max(np.abs(iq.astype(np.float64) - want))
        print(f"tx sm case {case} antenna {a}: max |d| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound


def test_transmitter_rejects_bad_pairs():
    pair = S.Pair(4, 1, (2, 2), (104, 104), nof_prb=6).abi()
    tb = np.zeros(13, np.uint8)
    for edit in (lambda p: setattr(p[1], "cw", 0), lambda p: setattr(p[0], "pmi", 3), lambda p: setattr(p[1], "rnti", 9),
                 lambda p: setattr(p[0], "tm", 2)):
        bad = S.Pair(4, 1, (2, 2), (104, 104), nof_prb=6).abi()
        edit(bad)
        with pytest.raises(RuntimeError):
            abi.tx_subframe_sm(bad, tb, tb)
    abi.tx_subframe_sm(pair, tb, tb)


# ------------------------------------------------------------------------------------------------ 4: reference end to end
@functools.lru_cache(None)
def e2e_front(seed, prec, mcs):
    pair, tbs, iqs = S.e2e_samples(seed, prec, mcs)
    return (pair, tbs) + S.front(pair, iqs)


@pytest.mark.parametrize("mcs", S.E2E_MCS, ids=lambda m: "qm%d_%d_qm%d_%d" % m)
@pytest.mark.parametrize("prec", S.PRECODERS, ids=lambda p: "tm%d_pmi%d" % p)
def test_reference_chain_decodes_both_codewords(prec, mcs):
    """6 PRB at 30 dB through a selective channel per antenna, estimates from R.chest: both CRCs pass and both
    payloads are the transmitted ones, seeds 0..5"""
    for seed in S.E2E_SEEDS:
        pair, tbs, grids, ces = e2e_front(seed, prec, mcs)
        for q, (ok, pay, _) in enumerate(S.decode(pair, S.pdsch_llr_sm(pair, grids, ces))):
            assert ok and np.array_equal(pay, tbs[q]), (seed, q)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_reference_chain_can_fail(seed):
    """a TM3 transmission detected as TM4 / 1 fails at least one CRC, and so does a pair descrambled with q swapped"""
    pair, tbs, grids, ces = e2e_front(seed, (3, 0), S.E2E_MCS[0])
    wrong = S.decode(pair, S.pdsch_llr_sm(pair, grids, ces, tm=4, pmi=1))
    assert not (wrong[0][0] and wrong[1][0])
    swapped = S.decode(pair, S.pdsch_llr_sm(pair, grids, ces, swap_q=True))
    assert not (swapped[0][0] and swapped[1][0])


# ------------------------------------------------------------------------------------------------ 5: the emulated chain
@pytest.mark.parametrize("prec", S.PRECODERS, ids=lambda p: "tm%d_pmi%d" % p)
def test_emulated_chain_decodes(prec):
    """emu_pdsch_llr_sm -> emu_decode_llr (the planner with the pair, rate de-matching, int16 turbo, TB assembly) on
    case 4's reference grids and estimates: payloads == the transmitted ones"""
    for seed in (0, 1, 2):
        pair, tbs, grids, ces = e2e_front(seed, prec, S.E2E_MCS[0])
        llrs = emu_llr_sm(pair, [U.f32c(g) for g in grids], [U.f32c(c) for c in ces])
        pays, ok = emu_decode(pair.abi(), llrs, "i16", "lane")
        for q in range(2):
            assert ok[q] == 1 and np.array_equal(pays[q], tbs[q]), (seed, q)


# ------------------------------------------------------------------------------------------------ HARQ operating point
def test_harq_point_reference():
    """Pins the scenario of the GPU HARQ test: at S.HARQ_SNR_DB codeword 1 (64QAM, rate 0.9) fails at rv 0 and passes
    once rv 2 is combined with it, while codeword 0 -- a new transport block in both transmissions -- passes each time"""
    (p0, tbs0, iq0), (p1, tbs1, iq1) = S.harq_samples()
    first = S.decode(p0, S.pdsch_llr_sm(p0, *S.front(p0, iq0)), n_its=4)
    assert first[0][0] and np.array_equal(first[0][1], tbs0[0]) and not first[1][0]
    l1 = S.pdsch_llr_sm(p1, *S.front(p1, iq1))
    alone = S.decode(p1, l1, n_its=4)
    assert alone[0][0] and np.array_equal(alone[0][1], tbs1[0]) and not alone[1][0]
    both = S.decode(p1, l1, soft=(None, first[1][2]), n_its=4)
    assert both[1][0] and np.array_equal(both[1][1], tbs1[1])
