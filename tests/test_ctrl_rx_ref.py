"""CPU: the antenna-combining PDCCH soft bits.  tests/ctrl_rx_ref.py (float64 numpy) equals the oracle with one
antenna; the host emulation of the two-antenna kernel (emu_pdcch_llr_rx: the kernel's own arithmetic, ctrl_rx_body.h)
agrees with it within 1e-4 relative, the bar test_gpu_ctrl.py holds PDCCH soft bits to; and the diversity fixture is
what it claims: neither antenna plane alone yields the DCI, the combined soft bits do."""
import functools

import numpy as np
import pytest

import ctrl_rx_ref as X
import oracle_lib as O
import pdsch_ref as R
import pdsch_ref_util as U
from helpers import rel_err
from srsue_amd import abi

SHAPES = [dict(cell_id=37, nof_prb=6, nof_ports=2, sf=4, cfi=2, ng=3), dict(cell_id=12, nof_prb=25, nof_ports=1, sf=7, cfi=1, ng=1)]


@functools.lru_cache(None)
def inputs(i, snr=10.0):
    """(ctrl cfg, grids [2, 14 W], ces [2, P, 14 W]) as float32-exact complex: random QPSK on every RE through a channel
    of its own per antenna (pdsch_ref_util.channel), AWGN at snr per RE; the estimates are the channels themselves"""
    kw = SHAPES[i]
    c = R.Cfg(cell_id=kw["cell_id"], nof_prb=kw["nof_prb"], nof_ports=kw["nof_ports"], sf=kw["sf"], cfi=kw["cfi"])
    q = O.ctrl_cfg(c.cell_id, c.nof_prb, c.nof_ports, kw["ng"], c.cfi, c.sf)
    tx = U.filled_grid(c, seed=i)
    H = [U.channel(c, 31 + 2 * i + a) for a in range(2)]
    grids = np.stack([U.rx_grid(tx, H[a], snr, 2 * i + a).reshape(-1) for a in range(2)]).astype(np.complex64)
    ces = np.stack([H[a].reshape(c.nof_ports, -1) for a in range(2)]).astype(np.complex64)
    return q, grids, ces


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["6prb_2p", "25prb_1p"])
def test_reference_with_one_antenna_is_the_oracle(built, i):
    q, grids, ces = inputs(i)
    kw = SHAPES[i]
    for a in range(2):
        want, n_cce = O.pdcch_llr(q, U.f32c(grids[a]), U.f32c(ces[a]))
        got, n = X.pdcch_llr_rx(q, grids[a:a + 1], ces[a:a + 1])
        assert n == n_cce and len(got) == len(want)
        assert rel_err(got, want) < 1e-6                   # the oracle returns float32
        emu = abi.emu_pdcch_llr_rx(kw["cell_id"], kw["nof_prb"], kw["nof_ports"], kw["ng"], kw["cfi"], kw["sf"],
                                   grids[a:a + 1], ces[a:a + 1])
        assert rel_err(emu, want) < 1e-4                   # one antenna: the emulation reduces to the oracle's operation


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["6prb_2p", "25prb_1p"])
@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_emulated_kernel_against_reference(built, i, noise):
    q, grids, ces = inputs(i)
    kw = SHAPES[i]
    for n_rx in (1, 2):
        want, _ = X.pdcch_llr_rx(q, grids[:n_rx], ces[:n_rx], noise)
        got = abi.emu_pdcch_llr_rx(kw["cell_id"], kw["nof_prb"], kw["nof_ports"], kw["ng"], kw["cfi"], kw["sf"],
                                   grids[:n_rx], ces[:n_rx], noise)
        assert len(got) == len(want)
        e = rel_err(got, want)
        print(f"emu pdcch llr n_rx {n_rx} {kw['nof_prb']} PRB noise {noise}: rel_err {e:.3e}")
        assert e < 1e-4
    # the second antenna matters: the combined soft bits are not antenna 0's
    assert rel_err(X.pdcch_llr_rx(q, grids[:1], ces[:1], noise)[0], want) > 1e-2


def test_emulation_rejects_bad_arguments(built):
    q, grids, ces = inputs(0)
    kw = SHAPES[0]
    with pytest.raises(ValueError):
        abi.emu_pdcch_llr_rx(kw["cell_id"], kw["nof_prb"], kw["nof_ports"], kw["ng"], 4, kw["sf"], grids, ces)
    with pytest.raises(ValueError):
        abi.emu_pdcch_llr_rx(kw["cell_id"], kw["nof_prb"], 1, kw["ng"], kw["cfi"], kw["sf"], grids, ces)


def test_diversity_fixture_needs_both_antennas(built):
    """Reference soft bits of each plane alone do not decode the DCI at its candidate (32 / 40 of the CCE's 72 coded
    bits are non-zero, fewer than the 47- / 44-bit block); the combined ones do, and so do the emulated kernel's."""
    for f in X.diversity_fixture():
        assert f["A"] + 16 == {"2": 47, "2A": 44}[f["fmt"]]
        lo = 72 * f["ncce"]
        for a, held in ((0, 32), (1, 40)):
            llr, n_cce = X.pdcch_llr_rx(f["q"], f["grids"][a:a + 1], f["ces"][a:a + 1])
            assert n_cce == f["n_cce"] and np.count_nonzero(llr[lo:lo + 72]) == held and held < f["A"] + 16
            assert np.count_nonzero(llr) == held
            ok, bits = X.dci_decode(llr, f["ncce"], 1, f["A"], f["rnti"])
            assert not ok, (f["fmt"], a)
        llr, _ = X.pdcch_llr_rx(f["q"], f["grids"], f["ces"])
        ok, bits = X.dci_decode(llr, f["ncce"], 1, f["A"], f["rnti"])
        assert ok and np.array_equal(bits, f["bits"])
        q = f["q"]
        emu = abi.emu_pdcch_llr_rx(q.cell.id, 6, 2, q.ng, q.cfi, q.sf, f["grids"], f["ces"])
        assert rel_err(emu, llr) < 1e-4
        ok, bits = X.dci_decode(emu, f["ncce"], 1, f["A"], f["rnti"])
        assert ok and np.array_equal(bits, f["bits"])
        # and the search finds it where it was put, as the second size of the UE-specific space
        sizes = (O.lib().or_dci_size(O.DCI_1A, 6), f["A"])
        got = X.search(llr, f["n_cce"], q.sf, f["rnti"], sizes)
        assert got is not None and got[0] == 1 and np.array_equal(got[1], f["bits"]) and got[2:] == (1, f["ncce"])
