"""CPU: sanity of the PBCH reference (tests/pbch_ref.py) the GPU PBCH tests compare against -- rate matching
repetition structure, RE list properties (36.211 6.6.4), transmit -> oracle OFDM RX identity, and the noiseless
round trip over every (ports, phase, frames combined)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pbch_ref as R

H2 = [0.8 + 0.3j, -0.4 + 0.5j]


def test_rate_matching_repeats_each_coded_bit_16_times_4_per_frame():
    tags = np.arange(3 * R.D, dtype=np.uint8)          # coded bit p carries the value p
    e = np.zeros(R.E, np.uint8)
    O.lib().or_conv_rm_tx(tags, R.D, R.E, e)
    assert np.array_equal(np.bincount(e, minlength=120), np.full(120, 16))
    for q in range(4):
        assert np.array_equal(np.bincount(e[R.NB * q:R.NB * (q + 1)], minlength=120), np.full(120, 4))
    # and the encoder's output is that arrangement of the coded bits
    bits = np.random.default_rng(1).integers(0, 2, 24).astype(np.uint8)
    ee = R.encode(bits, 2)
    d = np.array([ee[np.argmax(e == p)] for p in range(120)], np.uint8)
    assert np.array_equal(ee, d[e])


@pytest.mark.parametrize("nof_prb", [6, 15, 50])
@pytest.mark.parametrize("cell_id", [0, 1, 2, 301, 503])
def test_re_list_properties(cell_id, nof_prb):
    W = 12 * nof_prb
    re = R.re_list(cell_id, nof_prb)
    assert len(re) == 240 and len(set(re.tolist())) == 240
    l, k = re // W, re % W
    assert np.array_equal(np.bincount(l, minlength=11)[7:], [48, 48, 72, 72])
    assert k.min() == 6 * nof_prb - 36 and k.max() == 6 * nof_prb + 35
    assert np.all(np.diff(re.astype(np.int64)) > 0)      # symbol, then subcarrier
    # CRS of ports 0/1 (symbol 7) and 2/3 (symbol 8) sit on k = 6 m + (v + N_ID mod 6) mod 6, v in {0, 3}
    crs = (l <= 8) & (k % 3 == cell_id % 3)
    assert not crs.any()
    for ports in (1, 2):
        cell = O.Cell(cell_id, nof_prb, ports)
        pd = np.zeros(14 * W, np.uint32)
        n = O.lib().or_pdsch_re_list(C.byref(cell), 2, 0, np.ones(110, np.uint8), pd)
        assert n > 0 and not set(pd[:n].tolist()) & set(re.tolist())


@pytest.mark.parametrize("nof_prb,ports,phase", [(6, 1, 0), (6, 2, 3), (15, 2, 1), (50, 1, 2)])
def test_reference_tx_through_oracle_ofdm_rx(nof_prb, ports, phase):
    cell_id = 7 + phase
    bits = np.random.default_rng(phase).integers(0, 2, 24).astype(np.uint8)
    iq = R.tx(cell_id, nof_prb, ports, bits, phase, h=H2)
    W = 12 * nof_prb
    grid = np.zeros(2 * 14 * W, np.float32)
    O.lib().or_ofdm_rx(C.byref(O.Cell(cell_id, nof_prb, ports)), iq, grid)
    g = grid.view(np.complex64)
    lg = R.layer_grids(cell_id, nof_prb, bits, ports, phase)
    # the oracle's OFDM RX is an unnormalised DFT: grid = sqrt(N) h x for a transmitter scaled 1 / sqrt(N)
    want = sum(H2[p] * lg[p] for p in range(ports)) * np.sqrt(O.lib().or_symbol_sz(nof_prb))
    re = R.re_list(cell_id, nof_prb)
    assert np.max(np.abs(g[re] - want[re])) < 1e-5 * np.sqrt(np.mean(np.abs(want[re]) ** 2))
    assert np.max(np.abs(np.delete(g, re))) < 1e-5 * np.max(np.abs(want))      # nothing anywhere else


def frame_soft_bits(cell_id, tx_ports, bits, phase, snr_db=None, seed=0, rx_ports=2):
    """soft bits [2][480] of one 6-PRB frame: oracle subframe 0 + reference PBCH -> oracle front end"""
    cell = O.make_cell(cell_id, 6, tx_ports)
    oc = O.tx_cfg(cell, sf_idx=0, cfi=2, tm=2 if tx_ports == 2 else 1, tbs=200, qm=2, snr_db=300.0,
                  h=H2 if tx_ports == 2 else [H2[0], 0j])
    iq, _ = O.tx_subframe(oc, np.zeros(25, np.uint8))
    iq = R.awgn(iq + R.tx(cell_id, 6, tx_ports, bits, phase, h=H2), snr_db, seed)
    grid, ce = R.front(cell_id, 6, rx_ports, iq)
    return R.soft_bits(cell_id, 6, rx_ports, grid, ce)


@pytest.mark.parametrize("ports", [1, 2])
def test_reference_round_trip_noiseless(ports):
    cell_id = 150 + ports
    bits = R.mib_bits(50, 0, 2, 516)
    frames = [frame_soft_bits(cell_id, ports, bits, ph) for ph in range(4)]
    other = 3 - ports
    for phi in range(4):
        for f in range(1, phi + 2):
            cand = frames[phi - f + 1:phi + 1]
            ok, got = R.decode_job(cell_id, cand, ports, f, phi)
            assert ok and np.array_equal(got, bits), (phi, f)
            got = R.decode(cell_id, cand)
            assert got is not None and got[:3] == (ports, phi, 1) and np.array_equal(got[3], bits)
            # never under the other port count's hypothesis, whatever the phase
            for P, ff, pp in R.jobs(len(cand), (other,)):
                assert not R.decode_job(cell_id, cand, P, ff, pp)[0], (phi, f, ff, pp)
            # nor at another phase of the right hypothesis
            for P, ff, pp in R.jobs(len(cand), (ports,)):
                if pp != phi:
                    assert not R.decode_job(cell_id, cand, P, ff, pp)[0], (phi, f, ff, pp)
