"""CPU: the PUCCH host planner (mi_pucch_resource / mi_pucch_resource_n / mi_pucch_select, include/mi_ul.h) against
the reference's restatement (tests/pucch_ref.py), field for field over the whole configuration sweep, the 36.213
10.1 selection table, and every rejection."""
import ctypes as C

import numpy as np
import pytest

import pucch_ref as R
from srsue_amd import abi

NCS = {1: range(8), 2: (0, 2, 4, 6), 3: (0, 3, 6)}


def cfg_records(n_pucch, **kw):
    a = np.zeros(len(n_pucch), abi.PUCCH_CFG_DTYPE)
    for k, v in kw.items():
        a[k] = v
    a["n_pucch"] = n_pucch
    return a


@pytest.mark.parametrize("nof_prb", [6, 25])
@pytest.mark.parametrize("cell_id", [0, 17, 503])           # 503 mod 30 = 23: N_ID mod 30 differs from N_ID
def test_resources_match_reference_over_the_sweep(built, cell_id, nof_prb):
    checked = 0
    for sf in range(10):
        for gh in (0, 1):
            for delta in (1, 2, 3):
                for N_cs in NCS[delta]:
                    for n_rb_2 in (0, 1, 2):
                        for fmt in (R.F1A, R.F2):
                            # every n_pucch up to (and including) the first one rejected: m grows with n_pucch
                            hi = 36 * nof_prb + 2
                            ref = R.resource(cell_id=cell_id, nof_prb=nof_prb, sf_idx=sf, fmt=fmt, n_pucch=np.arange(hi),
                                             delta=delta, N_cs=N_cs, n_rb_2=n_rb_2, gh=gh)
                            n_ok = int(np.argmin(ref["ok"]))
                            assert ref["ok"][:n_ok].all() and not ref["ok"][n_ok]
                            got, n = abi.pucch_resource_n(cfg_records(
                                np.arange(n_ok + 1), cell_id=cell_id, nof_prb=nof_prb, sf_idx=sf, rnti=0x46, format=fmt,
                                delta_shift=delta, N_cs=N_cs, n_rb_2=n_rb_2, group_hopping=gh,
                                cqi_len=4 if fmt == R.F2 else 0))
                            assert n == n_ok, (sf, gh, delta, N_cs, n_rb_2, fmt, n, n_ok)
                            assert abi.last_error()
                            for f in ("n_prb", "n_prime", "n_oc", "n_cs"):
                                assert np.array_equal(got[f], ref[f][:n_ok]), (f, sf, gh, delta, N_cs, n_rb_2, fmt)
                            assert np.all(got["u"] == ref["u"][None, :])
                            checked += n_ok
    assert checked > 10000


def test_single_call_matches_the_array_call(built):
    kw = dict(cell_id=77, nof_prb=25, sf_idx=6, rnti=1, format=abi.PUCCH_1B, delta_shift=2, N_cs=4, n_rb_2=1,
              group_hopping=1, shortened=1)
    rec, n = abi.pucch_resource_n(cfg_records(np.arange(50), **kw))
    assert n == 50
    for i in (0, 5, 6, 49):
        r = abi.pucch_resource(abi.pucch_cfg(n_pucch=i, **kw))
        assert list(r.n_prb) == rec["n_prb"][i].tolist() and list(r.u) == rec["u"][i].tolist()
        assert list(r.n_prime) == rec["n_prime"][i].tolist() and list(r.n_oc) == rec["n_oc"][i].tolist()
        assert [list(x) for x in r.n_cs] == rec["n_cs"][i].tolist()


def test_select_follows_36213_10_1(built):
    kw = dict(n_cce=7, N_pucch_1=11, n_pucch_2=3, n_pucch_sr=29)
    S = lambda **k: abi.pucch_select(**dict(kw, **k))
    assert S(ack_len=1) == (abi.PUCCH_1A, 18)                      # ACK, 1 bit
    assert S(ack_len=2) == (abi.PUCCH_1B, 18)                      # ACK, 2 bits
    assert S(ack_len=1, sr=True) == (abi.PUCCH_1A, 29)             # ACK with positive SR
    assert S(ack_len=2, sr=True) == (abi.PUCCH_1B, 29)
    assert S(sr=True) == (abi.PUCCH_1, 29)                         # positive SR alone
    assert S(cqi_len=4) == (abi.PUCCH_2, 3)                        # CQI alone
    assert S(cqi_len=4, ack_len=1) == (abi.PUCCH_2A, 3)            # CQI with 1 ACK bit
    assert S(cqi_len=4, ack_len=2) == (abi.PUCCH_2B, 3)            # CQI with 2 ACK bits
    assert S(cqi_len=4, sr=True) == (abi.PUCCH_1, 29)              # CQI with positive SR: CQI dropped
    assert S(cqi_len=4, ack_len=1, sr=True) == (abi.PUCCH_1A, 29)
    assert S(cqi_len=4, ack_len=2, simul_cqi_ack_dropped=True) == (abi.PUCCH_1B, 18)
    assert S() is None                                             # nothing to send
    # a NULL resource pointer is allowed
    assert abi.lib().mi_pucch_select(1, 0, 0, 0, 7, 11, 3, 29, None) == abi.PUCCH_1A


BAD = [dict(delta_shift=0), dict(delta_shift=4), dict(N_cs=8), dict(delta_shift=2, N_cs=3), dict(delta_shift=3, N_cs=4),
       dict(n_pucch=36 * 6),                                       # m = nof_prb
       dict(format=abi.PUCCH_2, cqi_len=4, n_pucch=72),            # m = nof_prb
       dict(format=abi.PUCCH_2, cqi_len=4, shortened=1), dict(format=abi.PUCCH_2A, cqi_len=0),
       dict(format=abi.PUCCH_2B, cqi_len=12), dict(format=abi.PUCCH_2, cqi_len=13),
       dict(nof_prb=0), dict(nof_prb=7), dict(nof_prb=110)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_rejections_leave_the_result_untouched(built, bad):
    r = abi.PucchRes()
    C.memset(C.byref(r), 0xA5, C.sizeof(r))
    before = bytes(r)
    assert abi.lib().mi_pucch_resource(C.byref(abi.pucch_cfg(**bad)), C.byref(r)) == -1
    assert abi.last_error()
    assert bytes(r) == before
    good = abi.pucch_cfg(**{k: v for k, v in bad.items() if k in ("format",)}, cqi_len=4 if "format" in bad else 0)
    assert abi.lib().mi_pucch_resource(C.byref(good), C.byref(r)) == 0
