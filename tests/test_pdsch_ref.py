"""CPU: the oracle (oracle/*.c), the product's transmitter and the emulated kernel bodies held to tests/pdsch_ref.py, the
independent float64 numpy restatement of the PDSCH chain (see its docstring for what is spec and what is convention).

Bounds: bit-level stages are exact.  or_dft computes in double: 1e-10 relative.  Float32 outputs of the oracle
(IQ, grid, ce, LLR) carry one float32 rounding of a double result: IQ within 2 * 2^-23 * max |iq|, the receive stages
rel_err < 1e-6 (2^-24 times a peak-to-RMS ratio below 8)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pdsch_ref as R
import pdsch_ref_util as U
from helpers import oracle_dlsch, rel_err
from srsue_amd import abi

ALL_K = [int(k) for k in R.CB_SIZES]
K_CHUNKS = [ALL_K[i:i + 47] for i in range(0, 188, 47)]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def interleave(d):
    """reference d[3, K + 4] -> the oracle's triplet order with 2 = NULL"""
    t = d.T.reshape(-1).copy()
    t[t == R.NULL] = 2
    return t.astype(np.uint8)


def test_reference_imports_only_numpy():
    import ast
    tree = ast.parse(open(R.__file__).read())
    mods = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | \
        {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods == {"numpy"}


def test_cb_sizes_and_segmentation():
    assert len(ALL_K) == 188 and all(O.lib().or_cb_size(i) == k for i, k in enumerate(ALL_K))
    for tbs in (16, 40, 512, 6120, 6128, 7000, 12216, 36696, 75376, 40000, 61664):
        s, r = O.cbsegm(tbs), R.segment(tbs + 24)
        assert (s.C, s.Cp, s.Cm, s.Kp, s.Km, s.F) == (r["C"], r["Cp"], r["Cm"], r["Kp"], r["Km"], r["F"]), tbs


def test_crc_and_gold():
    rng = np.random.default_rng(1)
    for n in (1, 24, 40, 999, 6144):
        b = rng.integers(0, 2, n).astype(np.uint8)
        for gen, fn in ((R.CRC24A, "or_crc24a"), (R.CRC24B, "or_crc24b"), (R.CRC16, "or_crc16")):
            p = R.crc(b, gen)
            assert getattr(O.lib(), fn)(b, n) == int("".join(map(str, p)), 2)
    for ci in (1, 0x7FFFFFFF, 0x12345678 & 0x7FFFFFFF, (0x46 << 14) | (5 << 9) | 301):
        c = np.zeros(5000, np.uint8)
        O.lib().or_gold(ci, c, 5000)
        assert np.array_equal(c, R.gold(ci, 5000))


@pytest.mark.parametrize("chunk", range(4))
def test_turbo_encoder_all_k(chunk):
    """or_tcod and the product's host encoder == the reference for every K, without and with filler bits.  Twelve
    random blocks per K and F: two exchanged interleaver entries show in a block only when their bits differ."""
    rng = np.random.default_rng(chunk)
    for K in K_CHUNKS[chunk]:
        blocks = rng.integers(0, 2, (12, K)).astype(np.uint8)
        for F in (0, int(rng.integers(1, 33))):
            want = R.turbo_encode_many(blocks, *U.qpp()[K], F)
            for bits, w in zip(blocks, want):
                d = np.zeros(3 * (K + 4), np.uint8)
                assert O.lib().or_tcod(bits, K, F, d) == 0
                assert np.array_equal(d, interleave(w)), (K, F)
                assert np.array_equal(abi.turbo_encode(bits, K, F), d), (K, F)


@pytest.mark.parametrize("chunk", range(4))
def test_rate_matching_all_k(chunk):
    """or_rm_tx == the matrix interleaver + circular buffer for every K x rv x E in {0.4 N_cb, N_cb - 1, N_cb, 2.5 N_cb},
    with filler bits; random 0 / 1 streams, so a one-position error in the permutation or k0 shows."""
    rng = np.random.default_rng(10 + chunk)
    for K in K_CHUNKS[chunk]:
        F = int(rng.integers(1, 33))
        d = rng.integers(0, 2, (3, K + 4))
        d[:2, :F] = R.NULL
        dt = interleave(d)
        Ncb = int(O.lib().or_ncb(K))
        assert Ncb == 3 * 32 * -(-(K + 4) // 32)
        for rv in range(4):
            for E in (int(0.4 * Ncb), Ncb - 1, Ncb, int(2.5 * Ncb)):
                e = np.zeros(E, np.uint8)
                assert O.lib().or_rm_tx(dt, K, E, rv, e) == 0
                assert np.array_equal(e, R.rate_match(d, K, F, E, rv)), (K, F, rv, E)


def test_rate_dematching_inverts_the_index_map():
    """or_rm_rx (softbuffer in the w domain, HARQ combine) gives the decoder input the reference accumulates through its
    transmit index map, over two transmissions with wraps and punctures."""
    rng = np.random.default_rng(5)
    for K, F in ((40, 0), (544, 8), (3520, 32), (6144, 0)):
        Ncb = int(O.lib().or_ncb(K))
        sb = np.zeros(Ncb, np.float32)
        soft = None
        for t, (rv, E) in enumerate(((0, int(0.7 * Ncb)), (2, int(1.9 * Ncb)))):
            e = rng.integers(-50, 50, E).astype(np.float32)          # integers: float32 sums are exact
            out = np.zeros(3 * (K + 4), np.float32)
            O.lib().or_rm_rx(e, E, K, F, rv, int(t == 0), sb, out)
            soft, d = R.rate_dematch(e.astype(np.float64), K, F, rv, soft)
            assert np.array_equal(out.reshape(K + 4, 3).T, d.astype(np.float32)), (K, rv)


def test_rm_E():
    for C_ in range(1, 14):
        for NL in (1, 2):
            for Qm in (2, 4, 6):
                for Gp in (C_ * 50, C_ * 50 + 1, C_ * 77 + C_ - 1, C_ * 1000 + C_ // 2):
                    G = Gp * NL * Qm
                    Es = [R.rm_E(G, C_, Qm, NL, r) for r in range(C_)]
                    assert sum(Es) == G                                                  # 36.212: the E_r fill G
                    assert Es == [O.lib().or_rm_E(G, C_, Qm, NL, r) for r in range(C_)]


@pytest.mark.parametrize("cell_id", [0, 1, 2, 3, 4, 5, 503])
def test_crs_sequence_and_positions(cell_id):
    L = O.lib()
    for ns in range(20):
        for l in (0, 4):
            rs = np.zeros(440, np.float32)
            L.or_crs_seq(cell_id, ns, l, rs)
            want, _ = R.crs(cell_id, ns, l, 0, 110)
            assert np.array_equal(rs, U.f32c(want)), (ns, l)
    # positions: in a subframe without sync / PBCH holes the REs that or_pdsch_re_list leaves out of a non-control
    # pilot symbol are exactly the configured ports' CRS subcarriers
    for nprb in (6, 25):
        for ports in (1, 2):
            cell = O.make_cell(cell_id, nprb, ports)
            re = np.zeros(14 * 12 * nprb, np.uint32)
            n = L.or_pdsch_re_list(C.byref(cell), 1, 3, np.ones(110, np.uint8), re)
            used = np.zeros(14 * 12 * nprb, bool)
            used[re[:n]] = True
            used = used.reshape(14, -1)
            for l in (4, 7, 11):
                want = np.sort(np.concatenate([R.crs(cell_id, 0, l % 7, p, nprb)[1] for p in range(ports)]))
                assert np.array_equal(np.flatnonzero(~used[l]), want), (nprb, ports, l)


@pytest.mark.parametrize("nprb", [6, 15, 25, 50, 75, 100])
def test_pdsch_re_list(nprb):
    rng = np.random.default_rng(nprb)
    full = np.ones((2, nprb), bool)
    part = np.tile(rng.random(nprb) < 0.5, (2, 1))
    part[:, nprb // 2] = True
    dist = rng.random((2, nprb)) < 0.5
    dist[0, 0], dist[1, 0] = True, False
    for cid in (0, 4, 503):
        for ports in (1, 2):
            cell = O.make_cell(cid, nprb, ports)
            for cfi in (1, 2, 3):
                for sf in (0, 5, 3):
                    for slots in (full, part, dist):
                        cfg = R.Cfg(cell_id=cid, nof_prb=nprb, nof_ports=ports, sf=sf, cfi=cfi, prb_slots=slots)
                        re = np.zeros(14 * 12 * nprb, np.uint32)
                        n = O.lib().or_pdsch_re_list(C.byref(cell), cfi, sf, U.prb_mask_u8(cfg), re)
                        assert np.array_equal(re[:n], np.flatnonzero(cfg.re_mask())), (cid, ports, cfi, sf)
                        if slots is full:
                            assert abi.pdsch_G(U.to_abi(cfg)) == n * cfg.Qm
    assert not R.Cfg(nof_prb=6, cfi=1).re_mask()[1].any() and R.Cfg(nof_prb=15, cfi=1).re_mask()[1].any()


@pytest.mark.parametrize("N", [128, 256, 512, 1024, 1536, 2048])
def test_dft(N):
    rng = np.random.default_rng(N)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    xin = np.stack([x.real, x.imag], 1).reshape(-1)
    for inverse, want in ((0, np.fft.fft(x)), (1, np.fft.ifft(x) * N)):
        out = np.zeros(2 * N)
        O.lib().or_dft(xin, out, N, inverse)
        got = out[0::2] + 1j * out[1::2]
        assert np.max(np.abs(got - want)) / np.sqrt(np.mean(np.abs(want) ** 2)) < 1e-10


TX_CASES = [
    dict(cell_id=301, nof_prb=6, nof_ports=1, sf=0, cfi=1, tbs=208, Qm=2),
    dict(cell_id=7, nof_prb=15, nof_ports=2, sf=5, cfi=2, tbs=2856, Qm=4, rnti=0x1234),
    dict(cell_id=11, nof_prb=25, nof_ports=1, sf=4, cfi=3, tbs=7000, Qm=4, rv=2),
    dict(cell_id=2, nof_prb=50, nof_ports=2, sf=9, cfi=1, tbs=12960, Qm=6, rv=3),
    dict(cell_id=5, nof_prb=75, nof_ports=1, sf=6, cfi=3, tbs=9912, Qm=6, rv=1, dist=True),
    dict(cell_id=503, nof_prb=100, nof_ports=2, sf=0, cfi=2, tbs=36696, Qm=6),
]


def make_cfg(kw):
    kw = dict(kw)
    if kw.pop("dist", False):
        s = np.random.default_rng(kw["nof_prb"]).random((2, kw["nof_prb"])) < 0.6
        s[0, :2], s[1, :2] = (True, False), (False, True)
        kw["prb_slots"] = s
    return R.Cfg(**kw)


@pytest.mark.parametrize("case", range(len(TX_CASES)))
def test_transmitters_equal_reference_iq(case):
    """Noiseless or_tx_subframe and the product's mi_tx_subframe == the reference IQ to float32 rounding: every
    bit-level stage, the RE mapping, CRS, PCFICH, SFBC signs, the bin mapping (DC skip), scaling and CP lengths."""
    cfg = make_cfg(TX_CASES[case])
    tb = U.tb_bytes(case, cfg.tbs)
    h = [0.75 + 0.25j, -0.5 + 0.625j][:cfg.nof_ports]
    H = np.array(h)[:, None, None] * np.ones((cfg.nof_ports, R.NSYMB, cfg.W))
    want = U.ref_subframe(cfg, tb, H).astype(np.float64)
    bound = 2 * 2.0 ** -23 * np.max(np.abs(want))
    hh = h + [0j] * (2 - len(h))
    iq_o, G = O.tx_subframe(U.to_otx(cfg, hh), tb)
    assert G == cfg.G
    iq_p = abi.tx_subframe(U.to_abi(cfg), tb, h=hh, snr_db=300.0)
    for name, iq in (("oracle", iq_o), ("product", iq_p)):
        err = np.max(np.abs(iq.astype(np.float64) - want))
        print(f"tx {name} case {case}: max |d| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, name


RX_CASES = [
    dict(cell_id=301, nof_prb=6, nof_ports=1, sf=0, cfi=1, tbs=208, Qm=2),
    dict(cell_id=8, nof_prb=15, nof_ports=2, sf=5, cfi=2, tbs=2856, Qm=4),
    dict(cell_id=4, nof_prb=75, nof_ports=2, sf=9, cfi=3, tbs=9912, Qm=6, dist=True),
    dict(cell_id=3, nof_prb=100, nof_ports=1, sf=1, cfi=1, tbs=36696, Qm=6),
]


@pytest.mark.parametrize("case", range(len(RX_CASES)))
def test_oracle_receiver_equals_reference(case):
    """or_ofdm_rx, or_chest and or_pdsch_llr on a reference subframe through the selective channel at 25 dB.  Each stage
    is fed the float32 rounding of the reference's previous stage (what its C interface carries), so the difference
    is the stage's own: one float32 output rounding."""
    cfg = make_cfg(RX_CASES[case])
    iq = U.ref_subframe(cfg, U.tb_bytes(40 + case, cfg.tbs), U.channel(cfg, case), 25.0, case)
    cell = O.make_cell(cfg.cell_id, cfg.nof_prb, cfg.nof_ports)
    L = O.lib()
    n = R.NSYMB * cfg.W
    grid = np.zeros(2 * n, np.float32)
    L.or_ofdm_rx(C.byref(cell), iq, grid)
    rgrid = R.ofdm_rx(U.c128(iq), cfg.nof_prb)
    e_grid = rel_err(grid, ri(rgrid))
    g32 = U.f32c(rgrid)
    ce, met = np.zeros(2 * n * cfg.nof_ports, np.float32), np.zeros(5, np.float32)
    L.or_chest(C.byref(cell), cfg.sf, g32, ce, met)
    rce, rmet = R.chest(U.c128(g32).reshape(R.NSYMB, cfg.W), cfg.cell_id, cfg.nof_prb, cfg.nof_ports, cfg.sf)
    e_ce = rel_err(ce, ri(rce))
    e_met = float(np.max(np.abs(met - rmet) / np.abs(rmet)))
    c32 = U.f32c(rce)
    llr, G = np.zeros(6 * n, np.float32), C.c_uint32()
    L.or_pdsch_llr(C.byref(cell), cfg.cfi, cfg.sf, U.prb_mask_u8(cfg), cfg.Qm, cfg.rnti, cfg.tm, 0.01, g32, c32, llr,
                   C.byref(G), None)
    rllr = R.pdsch_llr(cfg, U.c128(g32).reshape(R.NSYMB, cfg.W), U.c128(c32).reshape(cfg.nof_ports, R.NSYMB, cfg.W))
    assert G.value == len(rllr)
    e_llr = rel_err(llr[:G.value], rllr)
    print(f"rx case {case}: grid {e_grid:.3e} ce {e_ce:.3e} metrics {e_met:.3e} llr {e_llr:.3e}")
    assert e_grid < 1e-6 and e_ce < 1e-6 and e_llr < 1e-6 and e_met < 1e-6


def ri(x):
    """complex array -> interleaved float64"""
    x = np.asarray(x).reshape(-1)
    return np.stack([x.real, x.imag], 1).reshape(-1)


def test_reference_chain_decodes_its_own_transmission():
    """The reference receiver (OFDM, channel estimation, equaliser, demapper, rate de-matching, turbo decoder) recovers
    the reference transmitter's TB through the selective channel: TM1 with filler bits and TM2."""
    for i, kw in enumerate((dict(cell_id=4, nof_prb=6, sf=2, tbs=512, Qm=2),
                            dict(cell_id=9, nof_prb=6, nof_ports=2, sf=5, tbs=328, Qm=4, cfi=2))):
        cfg = R.Cfg(**kw)
        tb = U.tb_bytes(70 + i, cfg.tbs)
        iq = U.ref_subframe(cfg, tb, U.channel(cfg, i), 25.0, i)
        ok, pay, _ = R.dlsch_decode(cfg, U.ref_front(cfg, iq)[3], U.qpp())
        assert ok and np.array_equal(pay, tb)


# every emulated schedule and arithmetic: the float and the int16 lane decoders (plain, crossed, crossed recompute), the
# packed decoder plain and with each form of its waterfall compaction, and the latency form (64 / 256 segments)
EMU_SCHEDS = [("gen", "lane"), ("gen", "x"), ("gen", "xr"), ("i16", "lane"), ("i16", "x"), ("i16", "xr"), ("i16", "p2"),
              ("i16", "p2_compact"), ("i16", "p2_store_w"), ("i16", "p2_rounds"), ("i16", "p2_segments8"),
              ("i16", "win64"), ("i16", "win256")]


def emu_decode(cfgs, llrs, mode, sched, max_its=4):
    arr = abi.cfg_array(cfgs)
    flat = np.ascontiguousarray(np.concatenate(llrs), np.float32)
    pay = np.zeros(sum(c.tbs // 8 for c in cfgs), np.uint8)
    ok, its = np.zeros(len(cfgs), np.uint32), np.zeros(len(cfgs), np.uint32)
    E = abi.emu()
    variant = sched[3:] if sched.startswith("p2_") else ""
    rounds = variant in ("rounds", "segments8")
    E.emu_set_tdec_i16(int(mode == "i16"))
    E.emu_set_tdec_x({"lane": 0, "x": 1, "xr": 2, "p2": 3}.get(sched.split("_")[0], 0))
    E.emu_set_tdec_win(int(sched[3:]) if sched.startswith("win") else 0)
    E.emu_set_tdec_compact(int(bool(variant)))
    E.emu_set_tdec_store_w(int(variant == "store_w" or rounds))
    E.emu_set_tdec_rounds(int(rounds))
    E.emu_set_tdec_seg(8 if variant == "segments8" else 0)
    try:
        assert E.emu_decode_llr(C.cast(arr, C.c_void_p), len(cfgs), flat.ctypes.data, max_its, pay.ctypes.data,
                                ok.ctypes.data, its.ctypes.data, None) == 0
    finally:
        for fn in ("i16", "x", "win", "compact", "store_w", "rounds", "seg"):
            getattr(E, "emu_set_tdec_" + fn)(0)
    offs = [E.emu_payload_offset(C.cast(arr, C.c_void_p), len(cfgs), i) for i in range(len(cfgs))]
    return [pay[o:o + c.tbs // 8] for o, c in zip(offs, cfgs)], ok


@pytest.mark.parametrize("mode,sched", EMU_SCHEDS)
@pytest.mark.parametrize("name", list(U.DECODE_CASES))
def test_emulated_kernels_decode_reference_llrs(name, mode, sched):
    """The emulated rate de-matching, turbo and TB-assembly kernel bodies on reference LLRs (float32) of 70 subframes
    with distinct RNTI and TB -- a full and a partial 64-lane group per code-block size, which the packed decoder
    pairs: payload == the transmitted TB, in every schedule and arithmetic.  Nothing here comes from the oracle."""
    cfgs, tbs, llrs = U.decode_case(name, U.N_CB)
    pays, ok = emu_decode([U.to_abi(c) for c in cfgs], llrs, mode, sched)
    for i in range(len(cfgs)):
        assert ok[i] == 1 and np.array_equal(pays[i], tbs[i]), i


@pytest.mark.parametrize("mode,sched", EMU_SCHEDS)
@pytest.mark.parametrize("name", list(U.HARQ_CASES))
def test_emulated_kernels_harq_sequence(name, mode, sched):
    """rv 0, 2, 3, 1 of one TB through the emulated kernel bodies with the softbuffer arena kept between the calls: the
    TB CRC fails with need - 1 transmissions and passes with need (test_harq_point_reference_and_oracle fixes need from
    the reference decoder), where the payload is the transmitted TB."""
    cfgs, tb, _, _, llrs, need = U.harq_case(name)
    abi.emu().emu_keep_softbuffer(1)
    try:
        for t in range(need):
            pays, ok = emu_decode([U.to_abi(cfgs[t], new_tb=int(t == 0))], [llrs[t]], mode, sched)
            assert bool(ok[0]) == (t == need - 1), t
    finally:
        abi.emu().emu_keep_softbuffer(0)
    assert np.array_equal(pays[0], tb)


@pytest.mark.parametrize("name", list(U.HARQ_CASES))
def test_harq_point_reference_and_oracle(name):
    """Fixes the HARQ operating points the GPU test uses: with rv 0, 2, 3, 1 combined, the reference decoder fails with
    need - 1 transmissions and recovers the TB with need; the oracle's decoders (both arithmetics, 4 iterations)
    fail and succeed at the same transmissions."""
    cfgs, tb, _, _, llrs, need = U.harq_case(name)
    soft, osb = None, {False: None, True: None}
    for t in range(need):
        ok, pay, soft = R.dlsch_decode(cfgs[t], llrs[t].astype(np.float64), U.qpp(), soft, n_its=4)
        assert ok == (t == need - 1), t
        for i16 in (False, True):
            ook, opay, _, osb[i16] = oracle_dlsch(U.to_abi(cfgs[t]), llrs[t], sb=osb[i16], new_tb=t == 0, i16=i16)
            assert ook == ok, (t, i16)
    assert np.array_equal(pay, tb) and np.array_equal(opay, tb)


@pytest.mark.parametrize("chunk", range(4))
def test_code_block_operating_points(chunk):
    """The two operating points test_gpu_pdsch_ref.py runs every code-block size at.  Easy point: both oracle decoders
    recover every one of the 70 CRC24A-carrying blocks of every K within 6 iterations (no block is left out).  Waterfall
    point: 4 iterations leave residual errors in part of the blocks."""
    wrong = 0
    for K in ALL_K[chunk::4]:
        bits, _ = U.blocks(K, True)
        for i16 in (False, True):
            obits, oits, ook = U.oracle_decisions(K, True, i16)
            assert ook.all() and np.array_equal(obits, bits) and oits.max() <= 6, (K, i16)
        wbits, _ = U.blocks(K, False)
        wrong += int((U.oracle_decisions(K, False, True)[0] != wbits).any(1).sum())
    assert 47 < wrong < 47 * 60


@pytest.mark.parametrize("K", [40, 104, 328])
def test_reference_decoder_reaches_what_the_oracle_reaches(K):
    """The textbook float64 decoder on BPSK / AWGN blocks around the waterfall: wherever or_decode_cb (float, 8
    iterations) returns the transmitted bits, so does the reference."""
    rng = np.random.default_rng(K)
    td = O.Tdec(O.TDEC_GEN)
    n_ok = 0
    for i in range(24):
        bits = rng.integers(0, 2, K).astype(np.uint8)
        d = R.turbo_encode(bits, *U.qpp()[K])
        s2 = 1.0 / (2 * (K / (3.0 * K + 12)) * 10 ** ((1.0 + 0.15 * i) / 10))
        y = (2.0 * d - 1.0) + rng.normal(0, np.sqrt(s2), d.shape)           # bit 1 -> +1: LLR > 0 means 1
        llr = (2.0 * y / s2).astype(np.float32)
        dec, _, _ = td.decode_cb(llr.T.reshape(-1), K, max_its=8, early_stop=False)
        if np.array_equal(dec, bits):
            n_ok += 1
            got, _ = R.turbo_decode(llr.astype(np.float64), *U.qpp()[K], n_its=8)
            assert np.array_equal(got, bits), i
    assert n_ok >= 8
