"""CPU: the variable-symbol-count PUSCH reference (tests/pusch_ref.py) against the oracle at n_srs = 0, where both
exist, and its own structure at n_srs = 1, where the oracle does not reach."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pusch_ref as P
from test_gpu_ul import CASES, mk, tb_of

REF_TOL = 1e-5      # a tenth of the UL suite's TOL = 1e-4: the reference's own error leaves the GPU its budget


def rel_err(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.fixture(scope="module")
def oracle(built):
    return O.lib()


def test_case_count():
    assert len(CASES) == 23


@pytest.mark.parametrize("i", range(len(CASES)))
def test_full_subframe_equals_the_oracle_bit_for_bit(oracle, i):
    """n_srs = 0: g (CQI then data) equals or_ulsch_encode, and the Q' values equal the oracle's"""
    oc = O.ul_cfg(**mk(CASES[i]))
    tb = tb_of(i, oc.tbs)
    r = P.resource(oc)
    assert (r["q_ack"], r["q_ri"], r["q_cqi"]) == (oracle.or_ack_qprime(C.byref(oc)), oracle.or_ri_qprime(C.byref(oc)),
                                                   oracle.or_cqi_qprime(C.byref(oc)))
    g = np.zeros(oracle.or_pusch_G(C.byref(oc)), np.uint8)
    H = oracle.or_ulsch_encode(C.byref(oc), tb, g)
    mine = P.ulsch_encode(oc, tb)
    assert H == len(mine) and np.array_equal(mine, g[:H])
    # n_symb_initial = 12 spelled out is the same thing
    assert P.resource(oc, 0, 12) == r


@pytest.mark.parametrize("i", range(len(CASES)))
def test_full_subframe_iq_equals_the_oracle(oracle, i):
    """n_srs = 0: IQ within 1e-5 RMS-relative of or_pusch_encode.  Largest observed over the 23 configurations: 0.0
    (the same primitives in the same order: the float32 results are identical)."""
    oc = O.ul_cfg(**mk(CASES[i]))
    tb = tb_of(i, oc.tbs)
    ref = np.zeros(2 * 15 * P.FFT_SIZE[oc.nof_prb], np.float32)
    assert oracle.or_pusch_encode(C.byref(oc), tb, ref) == 0
    e = rel_err(P.encode(oc, tb), ref)
    print("rel_err", i, e)
    assert e < REF_TOL


SHORT = [  # UCI of every kind over QPSK / 16QAM / 64QAM, Q'_ACK and Q'_RI at their 4 M caps, hopping
    dict(nof_prb=6, n_prb=2, L_prb=1, tbs=56, Qm=2, ack_len=1, ack=1, ioff=5),
    dict(nof_prb=25, n_prb=4, L_prb=3, tbs=104, Qm=2, ack_len=2, ack=1, ioff=14, ri_len=2, ri=2, ri_ioff=12),
    dict(nof_prb=25, n_prb=2, L_prb=20, tbs=6200, Qm=4, ack_len=2, ack=2, ioff=9, ri_len=1, ri=1, ri_ioff=5,
         cqi=[1, 0, 1, 1], cqi_ioff=9),
    dict(nof_prb=15, n_prb=0, L_prb=15, tbs=328, Qm=2, cqi=[1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0] * 3, cqi_ioff=15),
    dict(nof_prb=50, n_prb=4, L_prb=6, tbs=1000, Qm=6, n_prb1=30, ack_len=1, ack=0, ioff=12, ri_len=2, ri=3, ri_ioff=9),
]


@pytest.mark.parametrize("i", range(len(SHORT)))
@pytest.mark.parametrize("nsi", [0, 12])
def test_shortened_interleaver_structure(oracle, i, nsi):
    """n_srs = 1: every g symbol lands in exactly one cell of the M x 11 matrix, the HARQ-ACK / RI cells are those of
    5.2.2.8 (from the last row up in columns {2, 3, 8, 9} / {1, 4, 7, 10}, four per row), symbol 13 of the grid is
    empty and the 11 data symbols carry unit power"""
    oc = O.ul_cfg(cell_id=40 + i, sf_idx=i, rnti=0x50 + i, **SHORT[i])
    tb = tb_of(100 + i, oc.tbs)
    r = P.resource(oc, 1, nsi)
    M, Qm = 12 * oc.L_prb, oc.Qm
    assert r["n_symb"] == 11 and r["G"] == (11 * M - r["q_cqi"] - r["q_ri"]) * Qm
    assert sum(r["E"]) == r["G"] and all(e % Qm == 0 for e in r["E"])
    g = P.ulsch_encode(oc, tb, 1, nsi)
    y, src = P.interleave(oc, g, 1, nsi)
    assert y.shape == (M, 11, Qm)
    n_g = len(g) // Qm
    data = src[src >= 0]
    ack = np.argwhere(src == -2)
    ri = np.argwhere(src == -1)
    # g: symbol k in one cell at most, in row-major order; the ones missing are exactly those HARQ-ACK punctured
    assert len(np.unique(data)) == len(data) and np.all(np.diff(data) > 0)
    assert len(data) + len(ack) == n_g and len(ri) == r["q_ri"] and len(ack) == r["q_ack"]
    assert not np.any(src == -3)
    for cells, q, cols in ((ack, r["q_ack"], P.ACK_COLS), (ri, r["q_ri"], P.RI_COLS)):
        assert set(cells[:, 1].tolist()) <= set(cols)
        want = {(M - 1 - k // 4, (cols[0], cols[3], cols[2], cols[1])[k % 4]) for k in range(q)}
        assert {tuple(c) for c in cells.tolist()} == want
    # the cells hold g's bits where they come from g
    rows, cols = np.nonzero(src >= 0)
    assert np.array_equal(y[rows, cols], g.reshape(-1, Qm)[src[rows, cols]])
    gr = P.grid(oc, tb, 1, nsi)
    assert not np.any(gr[13])
    for l in range(13):
        n0 = oc.n_prb1 if (oc.hop and l >= 7) else oc.n_prb
        used = np.zeros(12 * oc.nof_prb, bool)
        used[12 * n0:12 * n0 + M] = True
        assert not np.any(gr[l][~used])
        p = np.sum(gr[l][used].astype(np.float64) ** 2, 1)
        if l % 7 == 3:
            assert np.allclose(p, 1.0, atol=1e-5)            # DMRS: unit modulus
        elif Qm == 2:
            assert abs(np.mean(p) - 1.0) < 1e-5              # the 1/sqrt(M) DFT keeps QPSK's unit power
    a, b = P.symbol_span(oc.nof_prb, 13)
    iq = P.encode(oc, tb, 1, nsi)
    assert b == 15 * P.FFT_SIZE[oc.nof_prb] and not np.any(iq[2 * a:]) and np.any(iq[2 * a - 2 * (b - a):2 * a])


def test_shortening_changes_the_q_primes_only_through_n_symb_initial(oracle):
    """Q'_ACK / Q'_RI scale with n_symb_initial, not with n_srs; Q'_CQI's cap follows n_srs"""
    oc = O.ul_cfg(nof_prb=25, n_prb=0, L_prb=20, tbs=6200, Qm=4, ack_len=2, ack=1, ioff=9, ri_len=1, ri=1, ri_ioff=5,
                  cqi=[1, 0, 1, 1], cqi_ioff=9)
    a = P.resource(oc, 0, 11)
    b = P.resource(oc, 1, 0)
    assert (a["q_ack"], a["q_ri"], a["q_cqi"]) == (b["q_ack"], b["q_ri"], b["q_cqi"])
    assert a["G"] - b["G"] == 240 * 4
    c = P.resource(oc, 1, 12)
    full = P.resource(oc, 0, 0)
    assert (c["q_ack"], c["q_ri"], c["q_cqi"]) == (full["q_ack"], full["q_ri"], full["q_cqi"])
    assert c["q_ack"] > b["q_ack"]
