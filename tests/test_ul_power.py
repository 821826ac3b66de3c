"""CPU: open-loop UL power control (mi_ul_pusch_power, mi_ul_pucch_power, mi_ul_srs_power; include/mi_ul.h, 36.213
5.1) against the closed forms in numpy float64 on the float32 parameters: each term on and off, the cap at P_CMAX,
the msg3 branch, Delta_TF at two TB sizes, h(n_CQI) at 3, 4 and 11 bits, both P_SRS_OFFSET forms."""
import numpy as np
import pytest

from srsue_amd import abi

RTOL = 1e-6
F = lambda x: float(np.float32(x))          # what the float32 field holds


def cfg(**kw):
    d = dict(p0_nominal_pusch=-85.0, alpha=0.7, p0_nominal_pucch=-105.0, delta_f_pucch=(-2.0, 1.0, 2.0, 3.0, -1.0),
             delta_preamble_msg3=4.0, p0_ue_pusch=-3.0, delta_mcs_based=0, acc_enabled=0, p0_ue_pucch=2.0, p_srs_offset=7.0)
    d.update(kw)
    return d


def pusch(d, PL, p0_pre, L, sum_Kr):
    msg3 = p0_pre != 0
    p0 = F(p0_pre) + F(d["delta_preamble_msg3"]) if msg3 else F(d["p0_nominal_pusch"]) + F(d["p0_ue_pusch"])
    alpha = 1.0 if msg3 else F(d["alpha"])
    tf = 10 * np.log10(2.0 ** (1.25 * sum_Kr / (144.0 * L)) - 1) if d["delta_mcs_based"] else 0.0
    return min(23.0, 10 * np.log10(L) + p0 + alpha * F(PL) + tf)


def pucch(d, PL, fmt, n_cqi):
    h = 10 * np.log10(n_cqi / 4.0) if fmt >= abi.PUCCH_2 and n_cqi >= 4 else 0.0
    df = {abi.PUCCH_1: 0, abi.PUCCH_1B: 1, abi.PUCCH_2: 2, abi.PUCCH_2A: 3, abi.PUCCH_2B: 4}
    f = F(d["delta_f_pucch"][df[fmt]]) if fmt in df else 0.0
    return min(23.0, F(d["p0_nominal_pucch"]) + F(d["p0_ue_pucch"]) + F(PL) + h + f)


def srs(d, PL, m_srs):
    off = -3.0 + F(d["p_srs_offset"]) if d["delta_mcs_based"] else -10.5 + 1.5 * F(d["p_srs_offset"])
    return min(23.0, off + 10 * np.log10(m_srs) + F(d["p0_nominal_pusch"]) + F(d["p0_ue_pusch"]) + F(d["alpha"]) * F(PL))


def close(got, want):
    assert np.isclose(got, want, rtol=RTOL, atol=0), (got, want)


@pytest.mark.parametrize("kw", [dict(), dict(alpha=0.0), dict(alpha=1.0), dict(p0_ue_pusch=0.0), dict(p0_nominal_pusch=0.0),
                                dict(delta_mcs_based=1), dict(acc_enabled=1)])
def test_pusch_terms(built, kw):
    d = cfg(**kw)
    c = abi.ul_power_cfg(**d)
    for PL in (0.0, 73.25, 101.5):
        for L in (1, 3, 25, 100):
            close(abi.ul_pusch_power(c, PL, 0.0, L, 6144), pusch(d, PL, 0.0, L, 6144))


def test_pusch_delta_tf_at_two_tb_sizes(built):
    """TB of 256 bits on 3 PRB (one code block of 280 bits with its CRC, BPRE = 0.65) and the largest UL TB on 100 PRB
    (13 code blocks of 5824 bits, BPRE = 5.26)"""
    d = cfg(delta_mcs_based=1)
    c, off = abi.ul_power_cfg(**d), abi.ul_power_cfg(**cfg())
    for L, sum_Kr in [(3, 280), (100, 13 * 5824)]:
        want = pusch(d, 60.0, 0.0, L, sum_Kr)
        close(abi.ul_pusch_power(c, 60.0, 0.0, L, sum_Kr), want)
        tf = 10 * np.log10(2.0 ** (1.25 * sum_Kr / (144.0 * L)) - 1)
        assert abs((want - abi.ul_pusch_power(off, 60.0, 0.0, L, sum_Kr)) - tf) < 1e-4
    assert 10 * np.log10(2.0 ** (1.25 * 280 / 432.0) - 1) < 0 < 10 * np.log10(2.0 ** (1.25 * 13 * 5824 / 14400.0) - 1)


def test_pusch_msg3_branch(built):
    """p0_preamble != 0 marks a grant of the random-access response: P0 = p0_preamble + delta_preamble_msg3, alpha = 1"""
    d = cfg(alpha=0.4)
    c = abi.ul_power_cfg(**d)
    got = abi.ul_pusch_power(c, 90.0, -104.0, 2, 0)
    close(got, pusch(d, 90.0, -104.0, 2, 0))
    close(got, 10 * np.log10(2) - 104.0 + 4.0 + 90.0)
    assert abs(abi.ul_pusch_power(c, 90.0, 0.0, 2, 0) - (10 * np.log10(2) - 88.0 + F(0.4) * 90.0)) < 1e-4


def test_cap_at_p_cmax(built):
    d = cfg()
    c = abi.ul_power_cfg(**d)
    assert abi.P_CMAX == 23.0
    assert pusch(d, 140.0, 0.0, 100, 0) == 23.0 and abi.ul_pusch_power(c, 140.0, 0.0, 100, 0) == 23.0
    assert abi.ul_pusch_power(c, 200.0, -100.0, 1, 0) == 23.0
    assert abi.ul_pucch_power(c, 140.0, abi.PUCCH_2B, 11, 2) == 23.0
    assert abi.ul_srs_power(c, 160.0, 96) == 23.0
    # just below the cap nothing is clipped
    close(abi.ul_pucch_power(c, 125.0, abi.PUCCH_1A, 0, 1), -105.0 + 2.0 + 125.0)


@pytest.mark.parametrize("fmt", range(6))
def test_pucch_delta_f_and_h(built, fmt):
    d = cfg()
    c = abi.ul_power_cfg(**d)
    for n_cqi in (0, 3, 4, 11):
        for PL in (0.0, 88.5):
            close(abi.ul_pucch_power(c, PL, fmt, n_cqi, 1), pucch(d, PL, fmt, n_cqi))
    base = -105.0 + 2.0 + 88.5
    want_df = [-2.0, 0.0, 1.0, 2.0, 3.0, -1.0][fmt]
    close(abi.ul_pucch_power(c, 88.5, fmt, 3, 1), base + want_df)                  # n_cqi < 4: h = 0
    close(abi.ul_pucch_power(c, 88.5, fmt, 4, 1), base + want_df)                  # h(4) = 0
    h11 = 10 * np.log10(11 / 4.0) if fmt >= abi.PUCCH_2 else 0.0
    close(abi.ul_pucch_power(c, 88.5, fmt, 11, 1), base + want_df + h11)
    # every term off
    z = abi.ul_power_cfg(**cfg(p0_nominal_pucch=0.0, p0_ue_pucch=0.0, delta_f_pucch=(0.0,) * 5))
    assert abi.ul_pucch_power(z, 0.0, fmt, 0, 0) == 0.0


@pytest.mark.parametrize("kw", [dict(), dict(delta_mcs_based=1), dict(p_srs_offset=0.0), dict(p_srs_offset=15.0),
                                dict(delta_mcs_based=1, p_srs_offset=15.0), dict(alpha=0.0), dict(p0_ue_pusch=0.0)])
def test_srs_terms_and_both_offset_forms(built, kw):
    d = cfg(**kw)
    c = abi.ul_power_cfg(**d)
    for PL in (0.0, 95.0):
        for m_srs in (4, 24, 96):
            close(abi.ul_srs_power(c, PL, m_srs), srs(d, PL, m_srs))
    # K_S = 1.25: -3 + pSRS-Offset dB; K_S = 0: -10.5 + 1.5 pSRS-Offset dB
    on, off = abi.ul_power_cfg(**cfg(delta_mcs_based=1, alpha=0.0)), abi.ul_power_cfg(**cfg(alpha=0.0))
    close(abi.ul_srs_power(on, 50.0, 4), -3.0 + 7.0 + 10 * np.log10(4) - 88.0)
    close(abi.ul_srs_power(off, 50.0, 4), -10.5 + 10.5 + 10 * np.log10(4) - 88.0)
