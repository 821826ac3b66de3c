"""CPU: the host side of PUSCH in SRS subframes (include/mi_ul.h, no device needed): mi_ul_pusch_resource against
the reference's 36.212 5.2.2.6 arithmetic (tests/pusch_ref.py), the mi_ul_pusch_n_srs truth table against a few
lines of Python, mi_ul_pusch_power_nsymb against its closed form, and the rejections."""
import itertools
import math

import numpy as np
import pytest

import oracle_lib as O
import pusch_ref as P
from srsue_amd import abi

# 36.211 Tables 5.5.3.2-1..-4, column b = 0: m_SRS,0 per srs-BandwidthConfig for N_RB <= 40, <= 60, <= 80, <= 110
M_SRS0 = {0: (36, 32, 24, 20, 16, 12, 8, 4), 1: (48, 48, 40, 36, 32, 24, 20, 16), 2: (72, 64, 60, 48, 48, 40, 36, 32),
          3: (96, 96, 80, 72, 64, 60, 48, 48)}
# 36.211 Table 5.5.3.3-1 (FDD): (T_SFC, offsets) of srs-SubframeConfig 0..14
CS = [(1, (0,)), (2, (0,)), (2, (1,)), (5, (0,)), (5, (1,)), (5, (2,)), (5, (3,)), (5, (0, 1)), (5, (2, 3)), (10, (0,)),
      (10, (1,)), (10, (2,)), (10, (3,)), (10, (0, 1, 2, 3, 4, 6, 8)), (10, (0, 1, 2, 3, 4, 5, 6, 8))]
# per L_prb a small and a large byte-aligned TB (C = 1 up to C = 8 code blocks)
TBS = {1: (32, 440), 2: (88, 904), 3: (144, 1384), 5: (256, 2280), 20: (1064, 9144), 36: (1928, 16416),
       100: (5352, 46888)}


@pytest.fixture(scope="module")
def lib(built):
    return abi.lib()


def band(nof_prb, bw_cfg):
    tab = 0 if nof_prb <= 40 else 1 if nof_prb <= 60 else 2 if nof_prb <= 80 else 3
    m0 = M_SRS0[tab][bw_cfg]
    lo = nof_prb // 2 - m0 // 2
    return lo, lo + m0


def want_n_srs(nof_prb, sfc, bw_cfg, sf, p0, p1, L, ue, rule):
    if rule == abi.PUSCH_SRS_OFF:
        return 0
    if ue:
        return 1
    T, offs = CS[sfc]
    if sf % T not in offs:
        return 0
    if rule == abi.PUSCH_SRS_ALL_CS:
        return 1
    lo, hi = band(nof_prb, bw_cfg)
    return int(any(p < hi and p + L > lo for p in (p0, p1)))


UCI = [dict(), dict(ack_len=2, ack=1, ioff=14, ri_len=2, ri=3, ri_ioff=12, cqi=[1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1],
                    cqi_ioff=15)]


@pytest.mark.parametrize("L_prb", sorted(TBS))
def test_resource_equals_the_reference(lib, L_prb):
    """G, Q'_ACK, Q'_RI, Q'_CQI, C and E[] over Qm x n_srs x n_symb_initial x UCI on/off x a small and a large TB"""
    nof_prb = 6 if L_prb <= 5 else 25 if L_prb <= 20 else 50 if L_prb <= 36 else 100
    n = rejected = 0
    for Qm, n_srs, nsi, uci, tbs in itertools.product((2, 4, 6), (0, 1), (0, 11, 12), UCI, TBS[L_prb]):
        kw = dict(nof_prb=nof_prb, n_prb=0, L_prb=L_prb, tbs=tbs, Qm=Qm, **uci)
        want = P.resource(O.ul_cfg(**kw), n_srs, nsi)
        if want["q_cqi"] + want["q_ri"] >= want["n_symb"] * 12 * L_prb:
            with pytest.raises(RuntimeError, match="PUSCH"):
                abi.ul_pusch_resource(abi.ul_cfg(n_srs=n_srs, n_symb_initial=nsi, **kw))
            assert uci       # only UCI can take every cell
            rejected += 1
            continue
        r = abi.ul_pusch_resource(abi.ul_cfg(n_srs=n_srs, n_symb_initial=nsi, **kw))
        got = dict(n_symb=r.n_symb, G=r.G, q_ack=r.q_ack, q_ri=r.q_ri, q_cqi=r.q_cqi, C=r.C, E=list(r.E)[:r.C])
        assert got == want, (kw, n_srs, nsi)
        assert not any(list(r.E)[r.C:])
        n += 1
    assert n + rejected == 3 * 2 * 3 * 2 * 2 and n >= 36 + 18      # every combination without UCI, every large TB


def test_zeroed_fields_plan_as_before(lib):
    """n_srs = n_symb_initial = 0 is the 12-symbol plan: G = (12 M - Q'_CQI - Q'_RI) Qm with the oracle's Q' values"""
    import ctypes as C
    kw = dict(nof_prb=25, n_prb=2, L_prb=20, tbs=3000, Qm=2, ack_len=1, ack=1, ioff=7, cqi=[0, 1, 1, 0], cqi_ioff=15,
              ri_len=1, ri=1, ri_ioff=12)
    oc = O.ul_cfg(**kw)
    r = abi.ul_pusch_resource(abi.ul_cfg(**kw))
    L = O.lib()
    assert (r.q_ack, r.q_ri, r.q_cqi) == (L.or_ack_qprime(C.byref(oc)), L.or_ri_qprime(C.byref(oc)),
                                          L.or_cqi_qprime(C.byref(oc)))
    assert r.n_symb == 12 and r.G == L.or_pusch_G(C.byref(oc)) - (r.q_cqi + r.q_ri) * 2


def test_n_srs_truth_table(lib):
    """25 PRB with bw_cfg 2: band 0..23, PRB 24 outside; 6 PRB with bw_cfg 7: band 1..4; every subframe config"""
    assert band(25, 2) == (0, 24) and band(6, 7) == (1, 5)
    n = 0
    for (nof_prb, bw_cfg), sfc, sf, rule, ue in itertools.product(((25, 2), (6, 7), (50, 3), (100, 0)), range(15),
                                                                   range(10), range(3), (0, 1)):
        last = nof_prb - 1
        for p0, p1, L in ((0, 0, 1), (last, last, 1), (last, 2, 1), (2, last, 1), (0, 0, nof_prb), (last - 1, last - 1, 2)):
            got = abi.ul_pusch_n_srs(nof_prb, sfc, bw_cfg, sf, p0, p1, L, ue, rule)
            assert got == want_n_srs(nof_prb, sfc, bw_cfg, sf, p0, p1, L, ue, rule), (nof_prb, bw_cfg, sfc, sf, rule, ue, p0, p1, L)
            n += 1
    assert n == 4 * 15 * 10 * 3 * 2 * 6


def test_n_srs_named_cases(lib):
    f = abi.ul_pusch_n_srs
    OV, ALL, OFF = abi.PUSCH_SRS_OVERLAP, abi.PUSCH_SRS_ALL_CS, abi.PUSCH_SRS_OFF
    # subframe_config 7: subframes 0, 1, 5, 6
    assert f(25, 7, 2, 1, 23, 23, 1, 0, OV) == 1          # the band's last PRB
    assert f(25, 7, 2, 1, 24, 24, 1, 0, OV) == 0          # PRB 24 alone is outside the band
    assert f(25, 7, 2, 1, 24, 24, 1, 0, ALL) == 1         # srsLTE's rule shortens it anyway
    assert f(25, 7, 2, 1, 24, 24, 1, 1, OV) == 1          # the UE's own SRS always shortens
    assert f(25, 7, 2, 3, 0, 0, 25, 0, OV) == 0 and f(25, 7, 2, 3, 0, 0, 25, 0, ALL) == 0   # not cell-specific
    assert f(25, 7, 2, 1, 24, 10, 1, 0, OV) == 1          # hopping: only slot 1 inside the band
    assert f(25, 7, 2, 1, 10, 24, 1, 0, OV) == 1          # only slot 0 inside
    assert f(6, 0, 7, 4, 0, 0, 1, 0, OV) == 0 and f(6, 0, 7, 4, 5, 5, 1, 0, OV) == 0   # 6 PRB: PRBs 0 and 5 outside
    assert f(6, 0, 7, 4, 0, 0, 2, 0, OV) == 1 and f(6, 0, 7, 4, 4, 4, 2, 0, OV) == 1
    assert f(25, 7, 2, 1, 0, 0, 25, 1, OFF) == 0
    # bad arguments
    for bad in ((7, 7, 2, 1, 0, 0, 1, 0, OV), (25, 15, 2, 1, 0, 0, 1, 0, OV), (25, 7, 8, 1, 0, 0, 1, 0, OV),
                (25, 7, 2, 10, 0, 0, 1, 0, OV), (25, 7, 2, 1, 0, 0, 0, 0, OV), (25, 7, 2, 1, 24, 0, 2, 0, OV),
                (25, 7, 2, 1, 0, 24, 2, 0, OV), (25, 7, 2, 1, 0, 0, 1, 0, 3), (6, 7, 6, 1, 0, 0, 1, 0, OV)):
        assert f(*bad) == -1, bad


POWER = dict(p0_nominal_pusch=-85.0, alpha=0.7, p0_ue_pusch=-3.0, delta_preamble_msg3=4.0)


def test_power_nsymb(lib):
    """N_RE = 12 L_prb n_symb_initial (36.213 5.1.1.1): 12 is mi_ul_pusch_power, 11 the closed form"""
    PL = 71.5
    for mcs_based, (L, sumK), p0_pre in itertools.product((0, 1), ((3, 280), (20, 6208), (1, 440)), (0.0, -104.0)):
        c = abi.ul_power_cfg(delta_mcs_based=mcs_based, **POWER)
        assert abi.ul_pusch_power_nsymb(c, PL, p0_pre, L, sumK, 12) == abi.ul_pusch_power(c, PL, p0_pre, L, sumK)
        got = abi.ul_pusch_power_nsymb(c, PL, p0_pre, L, sumK, 11)
        p0, alpha = (p0_pre + 4.0, 1.0) if p0_pre else (-88.0, float(np.float32(0.7)))
        dtf = 10 * math.log10(2 ** (1.25 * sumK / (12 * 11 * L)) - 1) if mcs_based else 0.0
        want = min(10 * math.log10(L) + p0 + alpha * PL + dtf, 23.0)
        assert got == np.float32(want), (mcs_based, L, sumK, p0_pre)
        full = abi.ul_pusch_power(c, PL, p0_pre, L, sumK)
        if mcs_based:
            assert got > full and full < 23.0                           # fewer REs, more bits per RE
        else:
            assert got == full
    assert abi.ul_pusch_power_nsymb(abi.ul_power_cfg(**POWER), PL, 0.0, 3, 280, 0) == 0.0


GOOD = dict(nof_prb=25, n_prb=0, L_prb=3, tbs=104, Qm=2)
BAD = [dict(n_srs=2), dict(n_symb_initial=10), dict(n_symb_initial=13), dict(n_srs=1, n_symb_initial=1),
       # a 64-bit CQI at the largest beta_offset on a tiny TB takes every cell of the 11 symbols
       dict(n_srs=1, cqi=[1, 0] * 32, cqi_ioff=15), dict(cqi=[1, 0] * 32, cqi_ioff=15)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v if not isinstance(v, list) else len(v)}" for k, v in b.items())
                                          for b in BAD])
def test_rejections(lib, bad):
    """host only: mi_ul_pusch_resource returns -1 with an error that begins PUSCH and leaves the output untouched"""
    abi.ul_pusch_resource(abi.ul_cfg(**GOOD))
    r = abi.UlRes()
    r.G = 0xABCD
    import ctypes as C
    c = abi.ul_cfg(**dict(GOOD, **bad))
    assert abi.lib().mi_ul_pusch_resource(C.byref(c), C.byref(r)) == -1
    assert abi.last_error().startswith("PUSCH")
    assert r.G == 0xABCD and r.n_symb == 0
