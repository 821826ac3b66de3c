"""GPU: DL control with two receive antennas and DCI formats 2 / 2A (mi_dl_ctrl_create_flags, mi_dci_dl2_*).

(a) combined PDCCH soft bits, PCFICH and PHICH against tests/ctrl_rx_ref.py (float64) and the host emulation
(b) blind search at the format 2 / 2A sizes, bit-exact on the oracle's soft bits
(c) the diversity fixture: a PDCCH that neither antenna holds alone
(d) from the air to the payload: the grant found over the air plans the decode of the pair it schedules

Bars: soft bits 1e-4 relative (helpers.rel_err), PHICH soft value 1e-3, CFI / verdicts / bits / payloads exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ctrl_rx_ref as X
import dci2_ref as D
import oracle_lib as O
from helpers import oracle_front, rel_err, tb_bytes
from srsue_amd import abi
from test_dci2_ref import FMT, tbs_qm, cfg_fields
from test_dl_grant import pack_1
from test_gpu_pdsch_ref import TOL, stream
from test_gpu_rx_div import iq_planes, plane_buffer, plane_part
from test_oracle_ctrl import tx_with_dci

pytestmark = pytest.mark.gpu

S_OFDM, S_CHEST = 1, 2
H_RX = ([0.9 + 0.2j, -0.3 + 0.5j], [0.4 - 0.6j, 0.7 + 0.3j])      # flat per-port channel of antenna 0 / 1


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert torch.cuda.is_available()


def pick_candidate(q, rnti, Lw, nth=-1):
    """(L, first CCE, n_cce) of a UE-specific candidate of aggregation level Lw (the largest below it if there is none)"""
    re, lg, n_cce = X.regs(q)
    Ls, nc = np.zeros(32, np.uint32), np.zeros(32, np.uint32)
    k = O.lib().or_search_space(n_cce, q.sf, rnti, 0, Ls, nc)
    cand = [j for j in range(k) if Ls[j] == Lw] or [j for j in range(k) if Ls[j] <= Lw]
    return int(Ls[cand[nth]]), int(nc[cand[nth]]), n_cce


def hf(h):
    return np.array([v for z in h for v in (z.real, z.imag)], np.float32)


def awgn(iq, snr_db, seed):
    if snr_db is None:
        return iq.astype(np.float32)
    rng = np.random.default_rng(seed)
    return (iq + rng.normal(0, np.sqrt(10 ** (-snr_db / 10) / 2), iq.shape)).astype(np.float32)


def front(cfgs, iqs, n_rx):
    """a batch after OFDM | CHEST; iqs[a][i]: antenna a's samples of entry i"""
    b = abi.Batch(cfgs, max_its=4, n_rx=n_rx)
    d = iq_planes(b, iqs)
    b.run_stages(S_OFDM | S_CHEST, d.data_ptr(), stream())
    torch.cuda.synchronize()
    return b, d


# ------------------------------------------------------------------------------------------------ (a) combining
A_CASES = [  # nof_prb, ports, cfi, ng, sf, snr, L, I_lowest, n_dmrs, ack
    (6, 2, 2, 3, 9, 10.0, 1, 2, 7, 0), (6, 2, 2, 3, 4, None, 2, 1, 3, 1),
    (25, 1, 1, 1, 1, 10.0, 2, 5, 1, 1), (25, 1, 1, 1, 6, None, 4, 11, 0, 0),
]


@functools.lru_cache(None)
def a_inputs():
    built = []
    for i, (nprb, ports, cfi, ng, sf, snr, Lw, il, nd, ack) in enumerate(A_CASES):
        rnti = 0x70 + i
        cfg = abi.sf_cfg(cell_id=5 + 9 * i, nof_prb=nprb, nof_ports=ports, sf_idx=sf, cfi=cfi, tbs=1000, Qm=2, rnti=rnti)
        q = O.ctrl_cfg(cfg.cell_id, nprb, ports, ng, cfi, sf)
        L, ncce, _ = pick_candidate(q, rnti, Lw)
        bits = np.zeros(64, np.uint8)
        A = O.lib().or_dci1a_pack(nprb, C.byref(O.Dci1a(0, nprb, 5 + i, i % 8, 1, i % 4, 1)), bits)
        grp, seq = O.phich_calc(nprb, ng, il, nd)
        iqs = []
        for a in range(2):
            h = H_RX[a][:ports]
            hh = hf(h)
            iq, _ = tx_with_dci(cfg, ng, rnti, L, ncce, bits[:A], h=h, snr_db=None, seed=40 + i)
            for g, sq, hi in ((grp, seq, ack), (grp, (seq + 3) % 8, 1 - ack)):
                assert O.lib().or_tx_phich(C.byref(q), g, sq, hi, hh.ctypes.data, iq) == 0
            iqs.append(awgn(iq, snr, 900 + 2 * i + a))
        built.append(dict(cfg=cfg, q=q, snr=snr, iqs=iqs, bits=bits[:A].copy(), L=L, ncce=ncce, il=il, nd=nd, ack=ack, grp=grp, seq=seq))
    return built


@pytest.mark.parametrize("ng", [3, 1], ids=["6prb_2p_cfi2", "25prb_1p_cfi1"])
def test_combined_soft_bits_pcfich_phich(ng):
    cases = [c for c in a_inputs() if c["q"].ng == ng]
    cfgs = [c["cfg"] for c in cases]
    b, d = front(cfgs, [[c["iqs"][a] for c in cases] for a in range(2)], 2)
    grid, ce = b.download(abi.BUF_GRID, np.float32), b.download(abi.BUF_CE, np.float32)
    ctl = abi.Ctrl(b, phich_ng=ng, combine=True)
    ctl.set_phich([c["il"] for c in cases], [c["nd"] for c in cases])
    ctl.run(stream())
    torch.cuda.synchronize()
    gl = ctl.llr()
    for s, c in enumerate(cases):
        cfg, q = c["cfg"], c["q"]
        W, P = 12 * cfg.nof_prb, cfg.nof_ports
        grids = np.stack([plane_part(b, abi.BUF_GRID, grid, a, s, 2 * 14 * W).view(np.complex64) for a in range(2)])
        ces = np.stack([plane_part(b, abi.BUF_CE, ce, a, s, 2 * P * 14 * W).view(np.complex64).reshape(P, -1) for a in range(2)])
        want, n_cce = X.pdcch_llr_rx(q, grids, ces)
        off = ctl.llr_offset(s)
        got = gl[off:off + len(want)]
        emu = abi.emu_pdcch_llr_rx(cfg.cell_id, cfg.nof_prb, P, ng, cfg.cfi, cfg.sf_idx, grids, ces)
        e_ref, e_emu = rel_err(got, want), rel_err(got, emu)
        print(f"(a) sf {s} {cfg.nof_prb} PRB {P} ports: llr rel_err ref {e_ref:.3e} emu {e_emu:.3e}")
        assert ctl.n_cce(s) == n_cce and e_ref < 1e-4 and e_emu < TOL
        if c["snr"] is not None:                                # with noise the antennas' soft bits differ: both are in them
            assert rel_err(X.pdcch_llr_rx(q, grids[:1], ces[:1])[0], want) > 1e-3
        cfi, found = ctl.result(s)
        assert cfi == cfg.cfi
        assert found is not None and found[0] == O.DCI_1A and np.array_equal(found[1], c["bits"]) and found[3] == c["ncce"]
        ack, soft = ctl.phich(s)
        ref = X.phich_soft_rx(q, grids, ces, c["grp"], c["seq"])
        print(f"(a) sf {s}: phich soft {soft:.5f} ref {ref:.5f}")
        assert ack == bool(c["ack"]) and abs(soft - ref) <= 1e-3 * max(1.0, abs(ref))
    ctl.close()
    # flags = 0 on the same two-antenna batch: plane 0's soft bits, those of a one-antenna batch fed antenna 0's samples
    plain = abi.Ctrl(b, phich_ng=ng)
    plain.run(stream())
    b1, d1 = front(cfgs, [[c["iqs"][0] for c in cases]], 1)
    one = abi.Ctrl(b1, phich_ng=ng)
    one.run(stream())
    torch.cuda.synchronize()
    assert plain.llr().any() and np.array_equal(plain.llr(), one.llr())
    for s in range(len(cases)):
        assert plain.result(s)[0] == one.result(s)[0] and plain.phich(s) == one.phich(s)
    with pytest.raises(RuntimeError, match="two-antenna"):
        abi.Ctrl(b1, phich_ng=ng, combine=True)
    for x in (plain, one, b, b1):
        x.close()


# ------------------------------------------------------------------------------------------------ (b) search
B_SUBFRAMES = [  # nof_prb, format, aggregation level, cfi
    (6, "2A", 1, 3), (6, "2", 2, 3), (25, "2A", 4, 2), (25, "2", 2, 3), (50, "2A", 8, 2), (50, "2", 1, 1),
    (100, "2A", 2, 1), (100, "2", 8, 3),
]
B_NG = 2


@functools.lru_cache(None)
def b_clean():
    """per subframe: (placeholder entries, ctrl cfg, rnti, noiseless samples, second size, format code); the last one a
    tm = 1 subframe with a format 1 DCI"""
    rng = np.random.default_rng(0xB5EA)
    out = []
    for i, (nprb, fmt, Lw, cfi) in enumerate(B_SUBFRAMES + [(25, "1", 2, 2)]):
        ports = 1 if fmt == "1" else 2
        rnti, sf = 0x200 + 7 * i, (i * 3 + 1) % 10
        cell = 40 + 11 * i
        q = O.ctrl_cfg(cell, nprb, ports, B_NG, cfi, sf)
        L, ncce, _ = pick_candidate(q, rnti, Lw)
        if fmt == "1":
            bits = np.array(pack_1(nprb, ("t0", 0x1555), 9, 2, 1, 0, 1), np.uint8)
            code = O.DCI_1
        else:
            bits = np.array(D.pack(nprb, D.random_grant(rng, fmt, nprb)), np.uint8)
            code = FMT[fmt]
        few = [1 if p < 2 else 0 for p in range(nprb)]           # placeholder grants: the search does not read them
        txc = abi.sf_cfg(cell_id=cell, nof_prb=nprb, nof_ports=ports, sf_idx=sf, cfi=cfi, tbs=1000, Qm=2, rnti=rnti)
        iq, _ = tx_with_dci(txc, B_NG, rnti, L, ncce, bits, h=H_RX[0][:ports], snr_db=None, seed=i)
        if fmt == "1":
            entries = [abi.sf_cfg(cell_id=cell, nof_prb=nprb, nof_ports=1, sf_idx=sf, cfi=cfi, tbs=256, Qm=2, rnti=rnti, prb=few)]
        else:
            tm = 3 if fmt == "2A" else 4
            entries = [abi.sf_cfg(cell_id=cell, nof_prb=nprb, nof_ports=2, sf_idx=sf, cfi=cfi, tm=tm, tbs=256, Qm=2, rnti=rnti,
                                  prb=few, cw=cw, pmi=1 if tm == 4 else 0) for cw in (0, 1)]
        out.append((entries, q, rnti, iq, len(bits), code, txc))
    return out


@pytest.mark.parametrize("snr", [-2.0, 0.0, 2.0])
def test_search_at_the_new_sizes_bit_exact(snr):
    """The oracle's soft bits (one antenna's front end) uploaded into the control object of a batch of tm 3 / tm 4 pairs
    and a tm 1 entry: per subframe the verdict, bits, L and first CCE equal a Python loop over or_search_space +
    or_dci_decode in the order 1A size, 2 / 2A (or 1) size, common 1A."""
    subs = b_clean()
    cfgs = [e for s in subs for e in s[0]]
    b = abi.Batch(cfgs, max_its=4, n_rx=2)
    ctl = abi.Ctrl(b, phich_ng=B_NG, tm_formats=True)
    legacy = abi.Ctrl(b, phich_ng=B_NG)
    flat = np.zeros(abi.lib().mi_dl_ctrl_llr_floats(ctl.h), np.float32)
    refs, first, jobs = [], [], 0
    Ls, nc = np.zeros(32, np.uint32), np.zeros(32, np.uint32)
    for i, (entries, q, rnti, iq, A2, code, txc) in enumerate(subs):
        first.append(sum(len(s[0]) for s in subs[:i]))
        grid, ce, _, _ = oracle_front(txc, awgn(iq, snr, 300 + i))
        ollr, n_cce = O.pdcch_llr(q, grid, ce)
        off = ctl.llr_offset(first[i])
        assert ctl.n_cce(first[i]) == n_cce
        if len(entries) == 2:                                  # the cw = 1 entry reports its partner's
            assert ctl.llr_offset(first[i] + 1) == off and ctl.n_cce(first[i] + 1) == n_cce
        flat[off:off + len(ollr)] = ollr
        refs.append(X.search(ollr, n_cce, q.sf, rnti, (O.lib().or_dci_size(O.DCI_1A, q.cell.nof_prb), A2)))
        jobs += 2 * sum(O.lib().or_search_space(n_cce, q.sf, rnti, common, Ls, nc) for common in (0, 1))
    assert ctl.n_jobs == jobs                                   # a pair counted once
    assert legacy.n_jobs == jobs + sum(2 * sum(O.lib().or_search_space(ctl.n_cce(first[i]), s[1].sf, s[2], common, Ls, nc)
                                               for common in (0, 1)) for i, s in enumerate(subs) if len(s[0]) == 2)
    ctl.set_llr(flat)
    ctl.run(stream(), mask=abi.Ctrl.SEARCH)
    torch.cuda.synchronize()
    nfound = 0
    for i, (entries, q, rnti, iq, A2, code, txc) in enumerate(subs):
        for e in range(len(entries)):
            _, got = ctl.result(first[i] + e)
            ref = refs[i]
            assert (got is None) == (ref is None), (i, e)
            if got is not None:
                nfound += 1
                assert got[0] == (O.DCI_1A, code)[ref[0]] and np.array_equal(got[1], ref[1]) and got[2:] == ref[2:], (i, e)
    print(f"(b) snr {snr}: {nfound} results found")
    if snr >= 2.0:                              # at 2 dB the L = 8 DCIs (50, 100 PRB) and the tm 1 entry's format 1 decode
        assert all(refs[i] is not None and refs[i][0] == 1 for i in (4, 7, 8))
    for x in (ctl, legacy, b):
        x.close()


# ------------------------------------------------------------------------------------------------ (c) diversity
def fixture_batch(fix, swap=False):
    cfgs = []
    for f in fix:
        q = f["q"]
        cfgs += [abi.sf_cfg(cell_id=q.cell.id, nof_prb=6, nof_ports=2, sf_idx=q.sf, cfi=q.cfi, tm=f["tm"], tbs=256, Qm=2,
                            rnti=f["rnti"], cw=cw, pmi=1 if f["tm"] == 4 else 0) for cw in (0, 1)]
    b = abi.Batch(cfgs, max_its=4, n_rx=2)
    order = (1, 0) if swap else (0, 1)
    for which, key in ((abi.BUF_GRID, "grids"), (abi.BUF_CE, "ces")):
        parts = [[np.ascontiguousarray(f[key][a]).reshape(-1).view(np.float32) for f in fix for _ in range(2)] for a in order]
        b.upload(which, plane_buffer(b, which, parts))
    return b


def test_diversity_fixture_on_the_gpu():
    """The fixture of test_ctrl_rx_ref.py uploaded into both planes: the combined control object finds both DCIs with
    their bits; an object that reads plane 0 alone finds nothing, whichever antenna's arrays plane 0 holds."""
    fix = X.diversity_fixture()
    b = fixture_batch(fix)
    ctl = abi.Ctrl(b, phich_ng=2, combine=True, tm_formats=True)
    ctl.run(stream(), mask=abi.Ctrl.LLR | abi.Ctrl.SEARCH)
    torch.cuda.synchronize()
    gl = ctl.llr()
    for s, f in enumerate(fix):
        want, _ = X.pdcch_llr_rx(f["q"], f["grids"], f["ces"])
        off = ctl.llr_offset(2 * s)
        assert rel_err(gl[off:off + len(want)], want) < 1e-4
        for e in (2 * s, 2 * s + 1):
            _, got = ctl.result(e)
            assert got is not None and got[0] == FMT[f["fmt"]] and np.array_equal(got[1], f["bits"]), (s, e)
            assert got[2:] == (1, f["ncce"])
    ctl.close()
    swapped = fixture_batch(fix, swap=True)
    for bb, kw in ((b, dict(tm_formats=True)), (b, dict()), (swapped, dict(tm_formats=True)), (swapped, dict())):
        c = abi.Ctrl(bb, phich_ng=2, **kw)
        c.run(stream(), mask=abi.Ctrl.LLR | abi.Ctrl.SEARCH)
        torch.cuda.synchronize()
        assert np.count_nonzero(c.llr()) > 0
        assert all(c.result(e)[1] is None for e in range(4)), kw
        c.close()
    # and the swapped planes combine to the same DCIs
    c = abi.Ctrl(swapped, phich_ng=2, combine=True, tm_formats=True)
    c.run(stream(), mask=abi.Ctrl.LLR | abi.Ctrl.SEARCH)
    assert all(np.array_equal(c.result(2 * s)[1][1], f["bits"]) for s, f in enumerate(fix))
    for x in (c, b, swapped):
        x.close()


# ------------------------------------------------------------------------------------------------ (d) air to payload
def tx_entries(base, nprb, g, tm, pmi, cw_tbs):
    """the transmitter's entries of grant g, written by hand (cw_tbs: the TB index of each codeword)"""
    prbs = D.alloc_prbs(nprb, g)
    mask = [1 if p in prbs else 0 for p in range(nprb)]
    out = []
    for qd, t in enumerate(cw_tbs):
        mcs, _, rv = g["tb"][t]
        tbs, qm = tbs_qm(mcs, len(prbs))
        out.append(abi.sf_cfg(cell_id=base.cell_id, nof_prb=nprb, nof_ports=2, sf_idx=base.sf_idx, cfi=base.cfi,
                              rnti=base.rnti, tm=tm, rv=rv, tbs=tbs, Qm=qm, new_tb=1, prb=mask, nl_td=2, cw=qd, pmi=pmi))
    return out


@pytest.mark.parametrize("nprb", [6, 25])
def test_from_the_air_to_the_payload(nprb):
    """IQ in -> PDCCH found with both antennas -> format 2 / 2A unpacked into the entries -> those entries decoded.
    A TM4 pair with codebook index 2, a TM3 pair with the TBs swapped and a single-TB 2A grant (transmit diversity),
    two antennas, 30 dB; the batch starts from placeholder grants of the right cell, subframe, CFI, RNTI and tm."""
    P = D.rbg_size(nprb)
    n_rbg = -(-nprb // P)
    part = (1 << n_rbg) - 1 if nprb == 6 else 0x1B6D & ((1 << n_rbg) - 1)        # 25 PRB: a partial RBG bitmap
    ng, cfi = 2, 2
    plan = [  # format, tm of the placeholder, tb, swap, pinfo -> tm, pmi, TB of each codeword
        ("2", 4, [(16, 1, 0), (9, 0, 0)], 0, 1, 4, 2, (0, 1)),
        ("2A", 3, [(7, 1, 0), (14, 1, 0)], 1, 0, 3, 0, (1, 0)),
        ("2A", 3, [(12, 0, 0), (0, 0, 1)], 0, 0, 2, 0, (0,)),
    ]
    place, want, tbs, iqs, dcis = [], [], [], [[], []], []
    for s, (fmt, ptm, tb, swap, pinfo, tm, pmi, cw_tbs) in enumerate(plan):
        rnti, sf = 0x90 + s, (1, 3, 8)[s]
        base = abi.sf_cfg(cell_id=60 + s, nof_prb=nprb, nof_ports=2, sf_idx=sf, cfi=cfi, rnti=rnti, tbs=0, Qm=2)
        g = dict(format=fmt, alloc_type=0, type0_alloc=part, type1_subset=0, type1_shift=0, type1_bitmap=0, tpc=s, harq=s + 2,
                 swap=swap, tb=tb, pinfo=pinfo)
        ent = tx_entries(base, nprb, g, tm, pmi, cw_tbs)
        tb_data = [tb_bytes(10 * s + k, e.tbs) for k, e in enumerate(ent)]
        q = O.ctrl_cfg(base.cell_id, nprb, 2, ng, cfi, sf)
        L, ncce, _ = pick_candidate(q, rnti, 2 if nprb == 6 else 4)
        bits = np.array(D.pack(nprb, g), np.uint8)
        for a in range(2):
            hh = hf(H_RX[a])
            if len(ent) == 2:
                iq = abi.tx_subframe_sm(ent, tb_data[0], tb_data[1], h=H_RX[a], snr_db=30.0, seed=77 + 2 * s + a)
            else:
                iq = abi.tx_subframe(ent[0], tb_data[0], h=H_RX[a], snr_db=30.0, seed=77 + 2 * s + a)
            assert O.lib().or_tx_pdcch(C.byref(q), rnti, L, ncce, bits, len(bits), hh.ctypes.data, iq) == 0
            iqs[a] += [iq, iq]                                  # the placeholder is a pair: one offset for both entries
        other = [1 if p % 2 == 0 else 0 for p in range(nprb)]
        place += [abi.sf_cfg(cell_id=base.cell_id, nof_prb=nprb, nof_ports=2, sf_idx=sf, cfi=cfi, rnti=rnti, tm=ptm, tbs=256,
                             Qm=2, prb=other, cw=cw, pmi=1 if ptm == 4 else 0) for cw in (0, 1)]
        want.append(ent)
        tbs.append(tb_data)
        dcis.append((fmt, bits, ncce))
    b, d = front(place, iqs, 2)
    ctl = abi.Ctrl(b, phich_ng=ng, combine=True, tm_formats=True)
    ctl.run(stream())
    torch.cuda.synchronize()
    decoded = []
    for s, (fmt, bits, ncce) in enumerate(dcis):
        cfi_got, got = ctl.result(2 * s)
        assert cfi_got == cfi and got is not None, s
        assert got[0] == FMT[fmt] and np.array_equal(got[1], bits) and got[3] == ncce
        ents = abi.dci2_to_cfgs(abi.dci2_unpack(got[0], nprb, got[1]), place[2 * s], new_tb=(1, 1))
        assert len(ents) == len(want[s])
        for x, y in zip(ents, want[s]):
            assert cfg_fields(x) == cfg_fields(y), s
        decoded += ents
    ctl.close()
    b.replan(abi.Plan().build(decoded), stream())
    b.run(d.data_ptr(), stream())                              # the physical subframes lie where they lay: the same samples
    torch.cuda.synchronize()
    pay, crc = b.download(abi.BUF_PAYLOAD, np.uint8), b.download(abi.BUF_TB_CRC, np.uint32)
    i = 0
    for s in range(len(plan)):
        for k in range(len(want[s])):
            assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs[s][k]), (s, k)
            i += 1
    assert i == len(decoded) == 5
    b.close()
