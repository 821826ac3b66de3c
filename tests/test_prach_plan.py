"""CPU: the PRACH host planner (srsue_amd/csrc/prach_host.cpp: mi_prach_resource_n, mi_prach_root, mi_prach_format,
mi_prach_send_tti; no device needed) against the independent reference of tests/prach_ref.py, and its rejections."""
import ctypes as C
import itertools

import numpy as np
import pytest

import prach_ref as R
from srsue_amd import abi

ROOTS = (0, 22, 24, 455, 456, 816, 820, 837)   # group edges, the wrap 837 -> 0, roots with no restricted shift
PREAMBLES = (0, 1, 63)
BANDS = [(p, fo) for p in R.NFFT for fo in (0, p - 6)]
CONFIGS = (3, 19, 41, 63)                       # one prach-ConfigIndex per format


def sweep():
    keys = ("zero_corr_zone", "high_speed", "root_seq_idx", "preamble_idx", "band", "config_idx")
    for v in itertools.product(range(16), (0, 1), ROOTS, PREAMBLES, BANDS, CONFIGS):
        d = dict(zip(keys, v))
        d["nof_prb"], d["freq_offset"] = d.pop("band")
        yield d


def records(dicts):
    a = np.zeros(len(dicts), abi.PRACH_CFG_DTYPE)
    for n in abi.PRACH_CFG_FIELDS:
        a[n] = [d[n] for d in dicts]
    return a


@pytest.fixture(scope="module")
def swept(built):
    cfgs = list(sweep())
    want = [R.resource(**d) for d in cfgs]
    return cfgs, want


def test_resource_n_matches_reference_on_every_field(swept):
    cfgs, want = swept
    good = [(d, w) for d, w in zip(cfgs, want) if w is not None]
    assert len(good) > 30000
    got, n = abi.prach_resource_n(records([d for d, _ in good]))
    assert n == len(good), (n, good[n][0], abi.last_error())
    for f in abi.PRACH_RES_FIELDS:
        exp = np.array([w[f] for _, w in good], np.uint32)
        bad = np.nonzero(got[f] != exp)[0]
        assert not len(bad), (f, good[bad[0]][0], int(got[f][bad[0]]), int(exp[bad[0]]))


def test_configurations_the_reference_rejects_are_rejected(swept):
    """zero_corr_zone 15 with high_speed, and every restricted configuration of the sweep whose 838 roots give fewer
    than 64 preambles: each stops mi_prach_resource_n at its own position"""
    cfgs, want = swept
    bad = {(d["zero_corr_zone"], d["high_speed"], d["root_seq_idx"]) for d, w in zip(cfgs, want) if w is None}
    assert {(15, 1, r) for r in ROOTS} <= bad
    few = sorted(b for b in bad if b[0] != 15)
    print("restricted configurations with fewer than 64 preambles:", few)
    good = dict(nof_prb=6, config_idx=0, root_seq_idx=0, zero_corr_zone=1, high_speed=0, freq_offset=0, preamble_idx=0)
    for zczc, hs, root in sorted(bad):
        d = dict(good, zero_corr_zone=zczc, high_speed=hs, root_seq_idx=root)
        _, n = abi.prach_resource_n(records([good, d, good]))
        assert n == 1 and "PRACH" in abi.last_error(), d


def test_root_table_matches_reference(built):
    assert [abi.prach_root(i) for i in range(838)] == R.ROOTS
    assert abi.prach_root(838) == -1 and abi.prach_root(0xFFFFFFFF) == -1


def test_format_matches_reference(built):
    for c in range(70):
        assert abi.prach_format(c) == R.preamble_format(c), c


def test_send_tti_matches_reference(built):
    for c, tti, allowed in itertools.product(range(64), range(20), (-1, 1, 7)):
        assert abi.prach_send_tti(c, tti, allowed) == R.send_tti(c, tti, allowed), (c, tti, allowed)
    # later frames repeat the pattern of the first two
    for c, tti in itertools.product((0, 9, 31, 63), range(10200, 10240)):
        assert abi.prach_send_tti(c, tti) == R.send_tti(c, tti % 20), (c, tti)


GOOD = dict(nof_prb=25, config_idx=3, root_seq_idx=22, zero_corr_zone=5, high_speed=0, freq_offset=4, preamble_idx=7)
BAD = [dict(nof_prb=7), dict(nof_prb=0), dict(config_idx=30), dict(config_idx=46), dict(config_idx=60),
       dict(config_idx=61), dict(config_idx=62), dict(config_idx=64), dict(root_seq_idx=838), dict(zero_corr_zone=16),
       dict(zero_corr_zone=15, high_speed=1), dict(freq_offset=20), dict(nof_prb=6, freq_offset=1), dict(freq_offset=0xFFFFFFFE),
       dict(preamble_idx=64)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_resource_rejects_and_leaves_the_output_untouched(built, bad):
    assert R.resource(**dict(GOOD, **bad)) is None and R.resource(**GOOD) is not None
    abi.prach_resource(abi.prach_cfg(**GOOD))
    r = abi.PrachRes(*([0xDEAD] * len(abi.PRACH_RES_FIELDS)))
    ret = abi.lib().mi_prach_resource(C.byref(abi.prach_cfg(**dict(GOOD, **bad))), C.byref(r))
    assert ret == -1 and abi.last_error().startswith("PRACH")
    assert all(getattr(r, f) == 0xDEAD for f in abi.PRACH_RES_FIELDS)
    with pytest.raises(RuntimeError, match="PRACH"):
        abi.prach_resource(abi.prach_cfg(**dict(GOOD, **bad)))


def test_resource_n_stops_at_the_first_rejection(built):
    cfgs = [GOOD, dict(GOOD, preamble_idx=8), dict(GOOD, config_idx=30), dict(GOOD, preamble_idx=9)]
    got, n = abi.prach_resource_n(records(cfgs))
    assert n == 2
    assert [int(v) for v in got["C_v"]] == [R.resource(**c)["C_v"] for c in cfgs[:2]]
