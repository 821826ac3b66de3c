"""CPU: DCI formats 2 / 2A (mi_dci_dl2_size / _pack / _unpack / _to_cfg, host only) against tests/dci2_ref.py, the
integer restatement of 36.212 5.3.3.1.5 / 5.3.3.1.5A and 36.213 7.1.6.1 / 7.1.6.2, and against batch entries built by
hand.  Sizes are the known answers of the specification for the six bandwidths."""
import ctypes as C

import numpy as np
import pytest

import dci2_ref as D
import oracle_lib as O
from srsue_amd import abi

FMT = {"2": abi.DCI_2, "2A": abi.DCI_2A}
SIZES = {"2": {6: 31, 15: 34, 25: 39, 50: 43, 75: 45, 100: 51}, "2A": {6: 28, 15: 31, 25: 36, 50: 41, 75: 42, 100: 48}}


def to_abi(g):
    return abi.dci2(format=FMT[g["format"]], alloc_type=g["alloc_type"], type0_alloc=g["type0_alloc"],
                    type1_subset=g["type1_subset"], type1_shift=g["type1_shift"], type1_bitmap=g["type1_bitmap"],
                    tpc_pucch=g["tpc"], harq_process=g["harq"], tb_cw_swap=g["swap"], tb=g["tb"], pinfo=g["pinfo"])


def ref_tuple(g):
    return (FMT[g["format"]], g["alloc_type"], g["type0_alloc"], g["type1_subset"], g["type1_shift"], g["type1_bitmap"],
            g["tpc"], g["harq"], g["swap"]) + tuple(tb + (int(D.tb_enabled(tb)),) for tb in g["tb"]) + (g["pinfo"],)


@pytest.mark.parametrize("fmt", ["2", "2A"])
def test_sizes_36212(built, fmt):
    for nprb, want in SIZES[fmt].items():
        assert D.size(fmt, nprb) == want
        assert abi.dci2_size(FMT[fmt], nprb) == want
    assert D.size("2A", 50) == 41 and 40 in D.AMBIGUOUS       # 40 padded to 41


@pytest.mark.parametrize("nprb", [6, 15, 25, 50, 75, 100])
def test_pack_unpack_against_reference(built, nprb):
    """300 seeded random valid grants per bandwidth: type 0 and type 1, both swap values, TB 1 or TB 2 disabled."""
    rng = np.random.default_rng(0xDC12 + nprb)
    seen = set()
    for i in range(300):
        fmt = "2" if i % 2 else "2A"
        g = D.random_grant(rng, fmt, nprb, disable=(None, None, 0, 1)[(i // 2) % 4])
        seen.add((g["alloc_type"], g["swap"], D.tb_enabled(g["tb"][0]), D.tb_enabled(g["tb"][1])))
        want = D.pack(nprb, g)
        d = to_abi(g)
        got = abi.dci2_pack(nprb, d)
        assert got.tolist() == want, (i, g)
        back = abi.dci2_unpack(FMT[fmt], nprb, got)
        assert back.as_tuple() == d.as_tuple() == ref_tuple(g), (i, g)
        assert D.unpack(fmt, nprb, want) == g
    types = {s[0] for s in seen}
    assert types == ({0, 1} if nprb > 10 else {0})
    assert {s[1] for s in seen} == {0, 1} and {s[2:] for s in seen} == {(True, True), (False, True), (True, False)}


def test_rejections(built):
    g = D.random_grant(np.random.default_rng(5), "2", 50, alloc_type=1)
    bits = np.array(D.pack(50, g), np.uint8)
    ok = abi.dci2_unpack(abi.DCI_2, 50, bits)
    assert ok.alloc_type == 1
    for bad in (bits[:-1], np.append(bits, 0)):                       # wrong nbits
        with pytest.raises(ValueError):
            abi.dci2_unpack(abi.DCI_2, 50, bad)
    with pytest.raises(ValueError):                                    # a format 2 payload is not a 2A payload
        abi.dci2_unpack(abi.DCI_2A, 50, bits)
    for ports in (1, 4):
        with pytest.raises(ValueError):
            abi.dci2_unpack(abi.DCI_2, 50, bits, nof_ports=ports)
        with pytest.raises(ValueError):
            abi.dci2_pack(50, to_abi(g), nof_ports=ports)
        with pytest.raises(ValueError):
            abi.dci2_size(abi.DCI_2, 50, ports)
    # 50 PRB: P = 3, two subset bits: subset 3 does not exist
    g3 = dict(g, type1_subset=3)
    with pytest.raises(ValueError):
        abi.dci2_unpack(abi.DCI_2, 50, np.array(D.pack(50, g3), np.uint8))
    with pytest.raises(ValueError):
        abi.dci2_pack(50, to_abi(g3))
    with pytest.raises(ValueError):
        abi.dci2_pack(25, to_abi(dict(g, type1_subset=2)))             # P = 2
    with pytest.raises(ValueError):
        abi.dci2_size(3, 50)                                           # not a format of this family
    with pytest.raises(ValueError):
        abi.dci2_pack(6, to_abi(dict(g, alloc_type=1)))                # no type 1 at N_RB <= 10
    with pytest.raises(ValueError):
        abi.dci2_pack(50, to_abi(dict(g, format="2A", pinfo=1)))       # format 2A has no precoding bits at 2 ports


# ---- to_cfg ------------------------------------------------------------------------------------------------------
def tbs_qm(mcs, n_prb):
    qm, itbs = C.c_uint32(), C.c_uint32()
    assert O.lib().or_mcs(mcs, C.byref(qm), C.byref(itbs)) == 0
    # the oracle holds the N_PRB = 6, 25, 50, 100 columns; the other columns are the table test_tables.py pins
    tbs = O.lib().or_tbs(itbs.value, n_prb)
    return (tbs if tbs > 0 else abi.lib().srslte_ra_tbs_from_idx(itbs.value, n_prb)), qm.value


def base_cfg(nprb, tm=2, **kw):
    return abi.sf_cfg(cell_id=11, nof_prb=nprb, nof_ports=2, sf_idx=3, cfi=2, rnti=0x51, tbs=0, Qm=2, tm=tm, **kw)


def cfg_fields(c):
    return tuple(getattr(c, n) for n, _ in abi.SfCfg._fields_ if n != "prb_mask") + (bytes(c.prb_mask),)


def by_hand(nprb, g, tm, pmi, cw_tbs, new_tb):
    """the entries a caller would write for grant g: cw_tbs = the TB index (0 / 1) carried by each codeword"""
    prbs = D.alloc_prbs(nprb, g)
    mask = [1 if p in prbs else 0 for p in range(nprb)]
    out = []
    for q, t in enumerate(cw_tbs):
        mcs, _, rv = g["tb"][t]
        tbs, qm = tbs_qm(mcs, len(prbs))
        out.append(abi.sf_cfg(cell_id=11, nof_prb=nprb, nof_ports=2, sf_idx=3, cfi=2, rnti=0x51, tm=tm, rv=rv, tbs=tbs,
                              Qm=qm, new_tb=new_tb[t], prb=mask, nl_td=2, cw=q, pmi=pmi))
    return out


def grant(fmt, nprb, tb, swap=0, pinfo=0, alloc_type=0, seed=1):
    g = D.random_grant(np.random.default_rng(seed), fmt, nprb, alloc_type=alloc_type, swap=swap)
    g["tb"], g["pinfo"] = list(tb), pinfo
    return g


TO_CFG_CASES = [
    # name, format, nprb, alloc type, tb, swap, pinfo, reported, -> tm, pmi, TB of each codeword
    ("2A pair", "2A", 25, 0, [(9, 1, 0), (17, 0, 2)], 0, 0, 0, 3, 0, (0, 1)),
    ("2A pair swapped, type 1", "2A", 50, 1, [(4, 0, 1), (28, 1, 3)], 1, 0, 0, 3, 0, (1, 0)),
    ("2 pair pinfo 0", "2", 6, 0, [(12, 1, 0), (3, 1, 0)], 0, 0, 0, 4, 1, (0, 1)),
    ("2 pair pinfo 1 swapped", "2", 100, 0, [(20, 0, 2), (20, 1, 1)], 1, 1, 0, 4, 2, (1, 0)),
    ("2 pair pinfo 2 reported 1", "2", 25, 1, [(0, 1, 0), (10, 1, 3)], 0, 2, 1, 4, 1, (0, 1)),
    ("2 pair pinfo 2 reported 2", "2", 75, 0, [(7, 0, 0), (27, 0, 0)], 0, 2, 2, 4, 2, (0, 1)),
    ("2A single TB 1", "2A", 25, 0, [(11, 1, 2), (0, 0, 1)], 1, 0, 0, 2, 0, (0,)),
    ("2A single TB 2", "2A", 15, 1, [(0, 1, 1), (22, 0, 0)], 0, 0, 0, 2, 0, (1,)),
    ("2 single, transmit diversity", "2", 50, 0, [(0, 0, 1), (16, 1, 1)], 0, 0, 0, 2, 0, (1,)),
]


@pytest.mark.parametrize("case", TO_CFG_CASES, ids=[c[0] for c in TO_CFG_CASES])
def test_to_cfg_matches_entries_built_by_hand(built, case):
    _, fmt, nprb, at, tb, swap, pinfo, reported, tm, pmi, cw_tbs = case
    g = grant(fmt, nprb, tb, swap, pinfo, at, seed=len(case[0]))
    new_tb = (1, 0)
    got = abi.dci2_to_cfgs(abi.dci2_unpack(FMT[fmt], nprb, np.array(D.pack(nprb, g), np.uint8)), base_cfg(nprb),
                           new_tb=new_tb, reported_cb_r2=reported)
    want = by_hand(nprb, g, tm, pmi, cw_tbs, new_tb)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert cfg_fields(a) == cfg_fields(b), [(n, getattr(a, n), getattr(b, n)) for n, _ in abi.SfCfg._fields_[:12]]
    abi.Plan().build(got)                                  # mi_dl_plan_build returns 0


REJECTS = [
    ("2 pair pinfo 2, nothing reported", "2", [(5, 0, 0), (5, 0, 0)], 2, 0, "reported"),
    ("2 pair pinfo 2, reported 3", "2", [(5, 0, 0), (5, 0, 0)], 2, 3, "reported"),
    ("2 pair pinfo 3", "2", [(5, 0, 0), (5, 0, 0)], 3, 1, "reserved"),
    ("2 pair pinfo 7", "2", [(5, 0, 0), (5, 0, 0)], 7, 1, "reserved"),
    ("2 single pinfo 1", "2", [(5, 0, 0), (0, 0, 1)], 1, 1, "rank-1 precoding is not built"),
    ("2 single pinfo 6", "2", [(0, 0, 1), (5, 0, 0)], 6, 1, "rank-1 precoding is not built"),
    ("2 single pinfo 7", "2", [(0, 0, 1), (5, 0, 0)], 7, 1, "reserved"),
    ("2A mcs 29", "2A", [(29, 0, 0), (5, 0, 0)], 0, 0, "MCS 29..31"),
    ("2 mcs 31 on the enabled TB", "2", [(0, 0, 1), (31, 0, 0)], 0, 0, "MCS 29..31"),
    ("2A both disabled", "2A", [(0, 0, 1), (0, 1, 1)], 0, 0, "disabled"),
]


@pytest.mark.parametrize("case", REJECTS, ids=[c[0] for c in REJECTS])
def test_to_cfg_rejections_leave_out_untouched(built, case):
    _, fmt, tb, pinfo, reported, text = case
    d = to_abi(grant(fmt, 25, tb, 0, pinfo))
    out = (abi.SfCfg * 2)()
    C.memset(out, 0xA5, C.sizeof(out))
    before = bytes(out)
    nt = np.array([1, 1], np.uint8)
    base = base_cfg(25)
    assert abi.lib().mi_dci_dl2_to_cfg(C.byref(d), C.byref(base), nt.ctypes.data, reported, C.cast(out, C.c_void_p)) == -1
    assert bytes(out) == before
    assert text in abi.last_error()


def test_to_cfg_rejects_bad_allocation_and_ports(built):
    out = (abi.SfCfg * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    before = bytes(out)
    nt = np.array([1, 1], np.uint8)
    call = lambda d, base: abi.lib().mi_dci_dl2_to_cfg(C.byref(d), C.byref(base), nt.ctypes.data, 0, C.cast(out, C.c_void_p))
    g = grant("2A", 50, [(5, 0, 0), (5, 0, 0)], alloc_type=1)
    assert call(to_abi(dict(g, type1_subset=3)), base_cfg(50)) == -1            # subset >= P
    assert call(to_abi(dict(g, alloc_type=0, type0_alloc=0)), base_cfg(50)) == -1   # nothing allocated
    one_port = abi.sf_cfg(cell_id=11, nof_prb=50, nof_ports=1, sf_idx=3, cfi=2, rnti=0x51, tbs=0, Qm=2)
    assert call(to_abi(g), one_port) == -1
    assert bytes(out) == before
