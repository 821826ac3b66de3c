"""CPU: the planner's view of spatial multiplexing (tm 3 / 4): a subframe is a cw 0 / cw 1 pair of entries over one
physical subframe.  Layout through the host emulation's emu_plan_info (the product's planner, plan.cpp), rejections
through mi_dl_plan_build with their mi_last_error text.  A plan of only TM1 / TM2 entries is pinned by
tests/test_plan.py, which must pass unchanged."""
import ctypes as C

import numpy as np
import pytest

import pdsch_ref as R
import pdsch_sm_ref as S
from srsue_amd import abi

NAMES = ("iq_off", "grid_off", "ce_off", "e_off", "G", "nre", "C", "E_sum", "E_min", "E_max", "pay_off", "in_fft",
         "iq_samples", "grid_elems", "ce_elems", "e_floats", "fft_entries", "chest_entries", "pairs", "max_units")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def info(cfgs, sf):
    arr = abi.cfg_array(cfgs)
    out = np.zeros(len(NAMES), np.uint64)
    assert abi.emu().emu_plan_info(C.cast(arr, C.c_void_p), len(cfgs), sf, out.ctypes.data) == 0, \
        abi.emu().emu_last_error().decode()
    return dict(zip(NAMES, (int(v) for v in out)))


def mixed_batch():
    """TM1 (15 PRB), a TM3 pair (6 PRB), TM2 (25 PRB), a TM4 pair (15 PRB, a second code block in codeword 1)"""
    tm1 = abi.sf_cfg(cell_id=3, nof_prb=15, nof_ports=1, sf_idx=2, cfi=2, tbs=1000, Qm=4)
    tm2 = abi.sf_cfg(cell_id=4, nof_prb=25, nof_ports=2, sf_idx=3, cfi=1, tbs=2024, Qm=2)
    p3 = S.Pair(3, 0, (4, 6), (1000, 1544), cell_id=5, nof_prb=6, sf=1, cfi=1)
    p4 = S.Pair(4, 2, (2, 6), (504, 7000), rv=(0, 2), cell_id=6, nof_prb=15, sf=4, cfi=3)
    return [tm1] + p3.abi() + [tm2] + p4.abi(), (p3, p4)


def test_pair_shares_its_subframe():
    cfgs, (p3, p4) = mixed_batch()
    I = [info(cfgs, s) for s in range(len(cfgs))]
    sf_len = lambda nprb: 15 * R.symbol_sz(nprb)
    phys = [0, 1, 3, 4]                                        # the entries that own samples
    assert I[0]["iq_samples"] == sum(sf_len(cfgs[s].nof_prb) for s in phys)
    assert I[0]["grid_elems"] == sum(14 * 12 * cfgs[s].nof_prb for s in phys)
    assert I[0]["ce_elems"] == sum(14 * 12 * cfgs[s].nof_prb * cfgs[s].nof_ports for s in phys)
    assert I[0]["fft_entries"] == 4 and I[0]["chest_entries"] == 4 and I[0]["pairs"] == 2
    for s0 in (1, 4):                                          # the cw = 1 entry sits on its partner's samples
        for k in ("iq_off", "grid_off", "ce_off"):
            assert I[s0 + 1][k] == I[s0][k], (s0, k)
        assert I[s0]["in_fft"] == 1 and I[s0 + 1]["in_fft"] == 0
    # running offsets over the physical subframes only
    iq = grid = ce = 0
    for s in phys:
        assert (I[s]["iq_off"], I[s]["grid_off"], I[s]["ce_off"]) == (iq, grid, ce), s
        iq += sf_len(cfgs[s].nof_prb)
        grid += 14 * 12 * cfgs[s].nof_prb
        ce += 14 * 12 * cfgs[s].nof_prb * cfgs[s].nof_ports
    # every entry is a transport block of its own: LLR range, payload, code blocks
    e = pay = 0
    for s in range(len(cfgs)):
        assert I[s]["e_off"] == e and I[s]["pay_off"] == pay, s
        e += (I[s]["G"] + 3) // 4 * 4
        pay += cfgs[s].tbs // 8
    assert I[0]["e_floats"] == e
    # the demap launch is sized by the TM1 / TM2 entries (units: REs, SFBC pairs)
    assert I[0]["max_units"] == max(I[0]["nre"], I[3]["nre"] // 2)


def test_pair_rate_matching_is_per_codeword():
    """N_L = 1 whatever nl_td says; G = nre Qm_q; the code blocks' E add up to G (36.212 5.1.4.1.2)"""
    cfgs, (p3, p4) = mixed_batch()
    for c in cfgs:
        c.nl_td = 2
    for s0, p in ((1, p3), (4, p4)):
        for q in range(2):
            i = info(cfgs, s0 + q)
            c = p.cw[q]
            assert i["nre"] == p.nre and i["G"] == p.nre * c.Qm
            sg = R.segment(c.tbs + 24)
            assert i["C"] == sg["C"] and i["E_sum"] == i["G"]
            Es = [R.rm_E(i["G"], sg["C"], c.Qm, 1, r) for r in range(sg["C"])]
            assert (i["E_min"], i["E_max"]) == (min(Es), max(Es))
    assert info(cfgs, 5)["C"] == 2


def test_zeroed_fields_plan_as_before():
    """cw = pmi = 0 on TM1 / TM2 entries: no pair, no channel-estimation list, every entry owns its samples"""
    cfgs = [abi.sf_cfg(cell_id=3, nof_prb=15, nof_ports=1 + i % 2, sf_idx=i, cfi=2, tbs=1000, Qm=4) for i in range(4)]
    assert all(c.cw == 0 and c.pmi == 0 for c in cfgs)
    i = info(cfgs, 3)
    assert i["pairs"] == 0 and i["chest_entries"] == 0 and i["fft_entries"] == 4 and i["in_fft"] == 1
    assert i["iq_samples"] == 4 * 15 * 256


def pair_with(**edits):
    p = S.Pair(edits.pop("tm", 4), edits.pop("pmi", 1), (2, 4), (104, 208), cell_id=9, nof_prb=6, sf=1, cfi=1).abi()
    for k, v in edits.items():
        q, name = int(k[-1]), k[:-1]
        if name == "prb_mask":
            p[q].prb_mask[0] = v
        else:
            setattr(p[q], name, v)
    return p


REJECTIONS = [
    # (cfgs, text of mi_last_error)
    (lambda: pair_with(nof_ports0=1, nof_ports1=1), "TM3 / TM4 need 2 ports"),
    (lambda: pair_with(tm=3, pmi=0, nof_ports0=1, nof_ports1=1), "TM3 / TM4 need 2 ports"),
    (lambda: pair_with()[1:], "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: [abi.sf_cfg(nof_prb=6, tbs=104, Qm=2)] + pair_with()[1:], "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with(rnti1=0x99), "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with(cfi1=2), "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with(sf_idx1=2), "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with(cell_id1=10), "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with(pmi1=2), "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with(tm=3, pmi=0, tm1=4, pmi1=1), "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with(prb_mask1=0), "cw = 1 entry must follow a matching cw = 0 entry"),
    (lambda: pair_with()[:1], "needs its cw = 1 partner"),
    (lambda: pair_with()[:1] + [abi.sf_cfg(nof_prb=6, tbs=104, Qm=2)], "needs its cw = 1 partner"),
    (lambda: pair_with()[:1] + pair_with(), "needs its cw = 1 partner"),
    (lambda: pair_with(pmi0=0, pmi1=0), "TM4 needs pmi 1 or 2"),
    (lambda: pair_with(pmi0=3, pmi1=3), "TM4 needs pmi 1 or 2"),
    (lambda: pair_with(cw1=2), "cw = 1 partner"),
    (lambda: [abi.sf_cfg(nof_prb=6, tbs=104, Qm=2, cw=1)], "cw and pmi must be 0 unless tm is 3 or 4"),
    (lambda: [abi.sf_cfg(nof_prb=6, nof_ports=2, tbs=104, Qm=2, pmi=1)], "cw and pmi must be 0 unless tm is 3 or 4"),
]


@pytest.mark.parametrize("case", range(len(REJECTIONS)))
def test_rejections(case):
    make, text = REJECTIONS[case]
    plan = abi.Plan()
    with pytest.raises(RuntimeError, match=text):
        plan.build(make())
    plan.build(pair_with() + pair_with(tm=3, pmi=0))       # the same object still plans a good batch
    plan.close()


def test_tm3_ignores_pmi_and_pairs_mix_with_other_modes():
    plan = abi.Plan()
    plan.build(pair_with(tm=3, pmi=0, pmi0=7, pmi1=7))
    plan.build(mixed_batch()[0])
    plan.close()
