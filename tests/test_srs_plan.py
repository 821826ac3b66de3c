"""CPU: the SRS host planner (mi_srs_resource / mi_srs_resource_n, include/mi_ul.h) against the reference's
restatement (tests/srs_ref.py), field for field over the whole configuration sweep, and every rejection."""
import ctypes as C

import numpy as np
import pytest

import srs_ref as R
from srsue_amd import abi

FIELDS = ("m_srs", "M_sc", "k0", "n_b", "n_SRS", "T_srs", "u", "v", "nzc", "q", "n_cs")
# one I_SRS per periodicity row of 36.213 Table 8.2-1 (first, last or inner), and for each tti 0, 10239 and values
# that straddle a change of n_SRS (k T - 1, k T)
I_SRS = [1, 2, 16, 17, 50, 156, 157, 636]
# (cell_id, group hopping, sequence hopping, delta_ss): 503 mod 30 = 23 differs from 503
CELLS = [(0, 0, 0, 0), (17, 1, 0, 0), (503, 0, 1, 7), (301, 1, 1, 29), (44, 0, 1, 0)]


def ttis(I):
    T = int(R.t_srs(I))
    return [0, T - 1, T, 3 * T - 1, 3 * T, 10239 - 10239 % T - 1, 10239 - 10239 % T, 10239]


def cfg_records(nof_prb, cell, I, tti, n_srs):
    g = np.meshgrid(np.arange(8), np.arange(4), np.arange(4), np.arange(24), np.arange(2), indexing="ij")
    bw, B, bh, nrrc, ktc = [a.ravel() for a in g]
    a = np.zeros(len(bw), abi.SRS_CFG_DTYPE)
    a["cell_id"], a["group_hopping"], a["sequence_hopping"], a["delta_ss"] = cell
    a["nof_prb"], a["tti"], a["I_srs"], a["n_srs"] = nof_prb, tti, I, n_srs
    a["bw_cfg"], a["B"], a["b_hop"], a["n_rrc"], a["k_tc"] = bw, B, bh, nrrc, ktc
    return a


@pytest.mark.parametrize("nof_prb", [6, 15, 25, 50, 75, 100])
def test_resources_match_reference_over_the_sweep(built, nof_prb):
    """all C_SRS x B x b_hop x n_RRC x k_TC of a bandwidth, for every (I_SRS, tti) above; the cell rotates"""
    checked, k = 0, 0
    for I in I_SRS:
        for tti in ttis(I):
            cell = CELLS[k % len(CELLS)]
            n_srs = k % 8
            k += 1
            a = cfg_records(nof_prb, cell, I, tti, n_srs)
            ref = R.resource(nof_prb=nof_prb, cell_id=cell[0], gh=cell[1], sh=cell[2], dss=cell[3], tti=tti, I_srs=I,
                             n_srs=n_srs, bw_cfg=a["bw_cfg"], B=a["B"], b_hop=a["b_hop"], n_rrc=a["n_rrc"],
                             k_tc=a["k_tc"])
            ok = ref["ok"]
            got, n = abi.srs_resource_n(a[ok])
            assert n == int(ok.sum()), (I, tti, n)
            for f in FIELDS:
                assert np.array_equal(got[f], ref[f][ok]), (f, I, tti, cell)
            # m_SRS,0 > nof_prb: the array call stops at the first such record
            if not ok.all():
                first = int(np.argmin(ok))
                _, stopped = abi.srs_resource_n(a)
                assert stopped == first and "m_SRS,0" in abi.last_error()
            checked += n
    assert checked > 6144 * (1 if nof_prb == 6 else 8)


def test_single_call_matches_the_array_call(built):
    a = cfg_records(100, (301, 1, 1, 29), 17, 4321, 5)
    rec, n = abi.srs_resource_n(a)
    assert n == len(a)
    for i in (0, 777, 3000, len(a) - 1):
        r = abi.srs_resource(abi.SrsCfg(*[int(a[i][f]) for f in abi.SRS_CFG_FIELDS]))
        for f in FIELDS:
            v = getattr(r, f)
            assert (list(v) if f == "n_b" else v) == rec[f][i].tolist(), f


GOOD = dict(cell_id=1, nof_prb=25, tti=7, bw_cfg=2, B=1, b_hop=0, n_rrc=3, k_tc=1, n_srs=2, I_srs=9)
# each field one past its range, the reserved I_SRS, m_SRS,0 > nof_prb, a bandwidth that is none of the six
BAD = [dict(cell_id=504), dict(tti=10240), dict(bw_cfg=8), dict(B=4), dict(b_hop=4), dict(n_rrc=24), dict(k_tc=2),
       dict(n_srs=8), dict(I_srs=637), dict(I_srs=1023), dict(delta_ss=30), dict(bw_cfg=1),
       dict(nof_prb=6, bw_cfg=6), dict(nof_prb=15, bw_cfg=4), dict(nof_prb=50, bw_cfg=8), dict(nof_prb=0),
       dict(nof_prb=7), dict(nof_prb=110)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_rejections_agree_and_leave_the_result_untouched(built, bad):
    kw = dict(GOOD, **bad)
    assert not R.valid(**{("dss" if k == "delta_ss" else k): v for k, v in kw.items()})
    r = abi.SrsRes()
    C.memset(C.byref(r), 0xA5, C.sizeof(r))
    before = bytes(r)
    assert abi.lib().mi_srs_resource(C.byref(abi.srs_cfg(**kw)), C.byref(r)) == -1
    assert abi.last_error().startswith("SRS")
    assert bytes(r) == before
    assert R.valid(**GOOD) and abi.lib().mi_srs_resource(C.byref(abi.srs_cfg(**GOOD)), C.byref(r)) == 0


def test_edges_of_every_range_are_accepted(built):
    for kw in [dict(cell_id=503), dict(tti=10239), dict(bw_cfg=7), dict(B=3), dict(b_hop=3), dict(n_rrc=23),
               dict(n_srs=7), dict(I_srs=636), dict(delta_ss=29), dict(nof_prb=6, bw_cfg=7), dict(nof_prb=15, bw_cfg=5)]:
        assert R.valid(**{("dss" if k == "delta_ss" else k): v for k, v in dict(GOOD, **kw).items()})
        abi.srs_resource(abi.srs_cfg(**dict(GOOD, **kw)))
