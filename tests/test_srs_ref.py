"""CPU: properties of the independent SRS reference (tests/srs_ref.py) alone -- the bandwidth tables, the frequency
position and its hopping pattern, the sequences against the oracle's PUSCH DMRS, orthogonality of the cyclic shifts
and of the combs.  The GPU tests compare the product with this reference."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import srs_ref as R

BW = [6, 15, 25, 50, 75, 100]


def test_table_quotients_are_integers():
    """N_b m_SRS,b = m_SRS,b-1 for every entry, m_SRS,3 = 4 everywhere, every m_SRS a multiple of 4"""
    m = R.M_SRS
    assert m.shape == (4, 4, 8)
    assert np.all(m[:, :-1] % m[:, 1:] == 0)
    N = m[:, :-1] // m[:, 1:]
    assert np.all(N * m[:, 1:] == m[:, :-1]) and np.all(N >= 1)
    assert np.all(m[:, 3] == 4) and np.all(m % 4 == 0)
    # the widest configuration of each table fits the widest bandwidth of its range
    assert [int(m[t, 0].max()) for t in range(4)] == [36, 48, 72, 96]
    assert [int(R.table_of(n)) for n in (6, 40, 41, 60, 61, 80, 81, 110)] == [0, 0, 1, 1, 2, 2, 3, 3]


def sweep(nof_prb, **kw):
    """every (C_SRS, B, b_hop, n_RRC, k_TC) of a bandwidth, as flat arrays"""
    g = np.meshgrid(np.arange(8), np.arange(4), np.arange(4), np.arange(24), np.arange(2), indexing="ij")
    bw, B, bh, nrrc, ktc = [a.ravel() for a in g]
    return dict(nof_prb=nof_prb, bw_cfg=bw, B=B, b_hop=bh, n_rrc=nrrc, k_tc=ktc, **kw)


@pytest.mark.parametrize("nof_prb", BW)
def test_occupied_band_lies_inside_the_cell(nof_prb):
    for I_srs, tti in [(0, 0), (0, 9), (7, 123), (400, 10239)]:
        r = R.resource(**sweep(nof_prb, I_srs=I_srs, tti=tti))
        ok = r["ok"]
        assert ok.any()
        assert np.all(r["k0"][ok] >= 0)
        assert np.all(r["k0"][ok] + 2 * (r["M_sc"][ok] - 1) < 12 * nof_prb)
        assert np.all(r["M_sc"][ok] <= R.NFFT[nof_prb] // 2)
    if nof_prb == 6:
        assert sorted(set(sweep(6)["bw_cfg"][ok].tolist())) == [7]


@pytest.mark.parametrize("nof_prb", BW)
def test_without_hopping_the_position_does_not_depend_on_tti(nof_prb):
    s = sweep(nof_prb, I_srs=0)
    off = s["b_hop"] >= s["B"]
    a, b = R.resource(**dict(s, tti=0)), R.resource(**dict(s, tti=4567))
    assert np.array_equal(a["k0"][off], b["k0"][off]) and np.array_equal(a["n_b"][off], b["n_b"][off])
    on = ~off & a["ok"]
    if nof_prb > 6:      # 6 PRB admits only C_SRS = 7, where every N_b is 1
        assert np.any(a["k0"][on] != b["k0"][on])


@pytest.mark.parametrize("nof_prb,bw_cfg", [(25, 2), (50, 0), (50, 1), (75, 0), (75, 2), (100, 0), (100, 1), (100, 2),
                                            (100, 5)])
def test_hopping_visits_every_position_once_and_tiles_the_hopping_bandwidth(nof_prb, bw_cfg):
    for B in range(1, 4):
        for b_hop in range(B):
            for n_rrc in (0, 5, 23):
                one = R.resource(nof_prb=nof_prb, bw_cfg=bw_cfg, B=B, b_hop=b_hop, n_rrc=n_rrc, I_srs=0, tti=0)
                period = int(np.prod(one["N_b"][0, b_hop + 1:B + 1]))
                # T_SRS = 2: n_SRS = tti // 2; start anywhere
                tti = 2 * (37 + np.arange(period))
                r = R.resource(nof_prb=nof_prb, bw_cfg=bw_cfg, B=B, b_hop=b_hop, n_rrc=n_rrc, I_srs=0, tti=tti)
                k0 = np.sort(r["k0"])
                width = 12 * int(r["m_srs"][0])
                assert len(set(k0.tolist())) == period
                assert np.all(np.diff(k0) == width)                 # adjacent, no gap, no overlap
                m_hop = int(R.M_SRS[R.table_of(nof_prb), b_hop, bw_cfg])
                assert period * width == 12 * m_hop                 # they tile the hopping bandwidth
                # ... which is the b_hop-level block that n_RRC selects
                fixed = R.resource(nof_prb=nof_prb, bw_cfg=bw_cfg, B=b_hop, b_hop=3, n_rrc=n_rrc, I_srs=0, tti=0)
                assert k0[0] == fixed["k0"][0]
                # and the next period repeats it
                r2 = R.resource(nof_prb=nof_prb, bw_cfg=bw_cfg, B=B, b_hop=b_hop, n_rrc=n_rrc, I_srs=0, tti=tti + 2 * period)
                assert np.array_equal(r["k0"], r2["k0"])


def test_periodicity_rows():
    assert R.t_srs([0, 1, 2, 6, 7, 16, 17, 36, 37, 76, 77, 156, 157, 316, 317, 636]).tolist() == [
        2, 2, 5, 5, 10, 10, 20, 20, 40, 40, 80, 80, 160, 160, 320, 320]
    r = R.resource(nof_prb=25, bw_cfg=2, I_srs=20, tti=[0, 19, 20, 10239])
    assert r["n_SRS"].tolist() == [0, 0, 1, 511] and r["T_srs"].tolist() == [20] * 4


@pytest.mark.parametrize("m_srs", sorted(set(R.M_SRS.ravel().tolist())))
def test_base_sequences_match_the_oracle_dmrs(m_srs):
    """v = 0 sequences of every SRS length against or_dmrs_pusch with L_prb = m_srs / 2 (cyclic shift divided out),
    groups 0, 13 and 29"""
    M = 6 * m_srs
    for u in (0, 13, 29):
        c = O.ul_cfg(cell_id=u, nof_prb=100, sf_idx=0, n_prb=0, L_prb=m_srs // 2, tbs=16, Qm=2)
        r = np.zeros(2 * M, np.float32)
        assert O.lib().or_dmrs_pusch(C.byref(c), 0, r) == 0
        a, b, ncs = C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert O.lib().or_dmrs_params(C.byref(c), 0, C.byref(a), C.byref(b), C.byref(ncs)) == 0
        assert (a.value, b.value) == (u, 0)
        z = (r[0::2].astype(np.float64) + 1j * r[1::2]) * np.exp(-2j * np.pi * ncs.value * np.arange(M) / 12)
        assert np.max(np.abs(z - R.base_seq(M, u, 0))) < 1e-6


def test_sequence_hopping_needs_72_subcarriers_and_no_group_hopping():
    # cell 7, delta_ss 3: c(ns) has both values over the ten odd slots
    c = R.c_seq(7, 3)[1::2]
    assert 0 < c.sum() < 10
    tti = np.arange(10)
    long = R.resource(nof_prb=15, bw_cfg=5, cell_id=7, sh=1, dss=3, tti=tti)      # M_sc = 72
    assert long["M_sc"][0] == 72 and long["v"].tolist() == c.tolist()
    short = R.resource(nof_prb=15, bw_cfg=6, cell_id=7, sh=1, dss=3, tti=tti)    # M_sc = 48
    assert short["M_sc"][0] == 48 and not short["v"].any()
    assert not R.resource(nof_prb=15, bw_cfg=5, cell_id=7, sh=1, gh=1, dss=3, tti=tti)["v"].any()
    # delta_ss moves c_init and not u
    assert np.array_equal(long["u"], R.resource(nof_prb=15, bw_cfg=5, cell_id=7, sh=1, dss=0, tti=tti)["u"])
    assert long["u"][0] == 7
    # v changes the root by one
    q0 = R.resource(nof_prb=15, bw_cfg=5, cell_id=7, sh=0, dss=3, tti=tti)["q"]
    assert np.array_equal(np.abs(long["q"] - q0), long["v"])


@pytest.mark.parametrize("nof_prb,bw_cfg,B", [(6, 7, 0), (15, 5, 0), (100, 0, 0), (100, 0, 3)])
def test_cyclic_shifts_are_orthogonal_and_combs_disjoint(nof_prb, bw_cfg, B):
    cfgs = [dict(nof_prb=nof_prb, bw_cfg=bw_cfg, B=B, cell_id=21, n_srs=n, k_tc=0, tti=3) for n in range(8)]
    grids = [R.grid(c) for c in cfgs]
    V = np.stack([g[13] for g in grids])
    G = np.abs(V @ V.conj().T)
    M = 6 * int(R.M_SRS[R.table_of(nof_prb), B, bw_cfg])
    assert np.allclose(np.diag(G), M)
    np.fill_diagonal(G, 0)
    assert G.max() < 1e-9 * M
    other = R.grid(dict(cfgs[0], k_tc=1))
    assert not np.any((np.abs(grids[0]) > 0) & (np.abs(other) > 0))
    assert np.count_nonzero(other) == M and not np.any(other[:13])


def test_reference_receiver_on_the_reference_transmitter():
    cfg = dict(nof_prb=25, bw_cfg=2, B=1, b_hop=0, n_rrc=3, k_tc=1, n_srs=5, cell_id=99, gh=1, tti=42)
    m = R.receive(R.demod(R.iq(cfg), 25), cfg)
    assert m["p_early"] < 1e-10 and abs(m["rms"] - 1) < 1e-5 and m["leak"] < 1e-5
    assert abs(m["h"] - 1) < 1e-5
    assert m["corr"][5] > 0.999 and np.all(np.delete(m["corr"], 5) < 1e-5)
