"""GPU: two-antenna receive diversity of the batched receiver (mi_dl_batch_create_rx) against tests/pdsch_rx_ref.py.

Float stages at the project's 1e-4 through helpers.rel_err, channel metrics at 2e-3, decoder outputs exact.

(a) front end per antenna plane  (b) demap alone against the combining reference  (c) fused == unfused, bit for bit
(d) one antenna through the new entry point == mi_dl_batch_create  (e) diversity end to end  (f) API edges."""
import numpy as np
import pytest
import torch

import pdsch_ref as R
import pdsch_ref_util as U
import pdsch_rx_ref as X
from helpers import rel_err
from srsue_amd import abi
from test_gpu_pdsch_ref import MET_TOL, TOL, chain_inputs, demap_cfgs, plain_cfg, ri, stream

pytestmark = pytest.mark.gpu

S_OFDM, S_CHEST, S_DEMAP, S_RM, S_TDEC, S_TB = (1 << i for i in range(6))


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert torch.cuda.is_available()


def iq_planes(b, iqs, dtype=np.float32):
    """the batch's IQ buffer (interleaved I/Q): iqs[a][i] at subframe i's offset in antenna a's plane"""
    flat = np.zeros(2 * len(iqs) * b.iq_samples, dtype)
    for a, per_sf in enumerate(iqs):
        for i, iq in enumerate(per_sf):
            o = 2 * (b.iq_offset(i) + a * b.iq_rx_stride)
            flat[o:o + len(iq)] = iq
    return torch.from_numpy(flat).cuda()


def plane_buffer(b, which, parts, scale=2):
    """the batch's whole buffer `which`: parts[a][i] at subframe i's offset in antenna a's plane"""
    flat = np.zeros(abi.lib().mi_dl_batch_bytes(b.h, which) // 4, np.float32)
    for a, per_sf in enumerate(parts):
        for i, p in enumerate(per_sf):
            o = scale * (b.offset(which, i) + a * b.rx_stride(which))
            flat[o:o + len(p)] = p
    return flat


def plane_part(b, which, buf, a, i, n, scale=2):
    o = scale * (b.offset(which, i) + a * b.rx_stride(which))
    return buf[o:o + n]


# ------------------------------------------------------------------------------------------------ (a) front end
def check_front(cfgs, iqs, sc16=False):
    """OFDM | CHEST of a two-antenna batch: every antenna's grid, ce and metrics == the reference front end of that
    antenna's samples"""
    b = abi.Batch([U.to_abi(c) for c in cfgs], n_rx=2, iq_sc16=sc16)
    assert b.n_rx == 2 and b.iq_rx_stride == b.iq_samples
    assert abi.lib().mi_dl_batch_bytes(b.h, abi.BUF_GRID) == 2 * 8 * b.rx_stride(abi.BUF_GRID)
    assert b.rx_stride(abi.BUF_METRICS) == len(cfgs) and b.rx_stride(abi.BUF_LLR) == 0
    d = iq_planes(b, iqs, np.int16 if sc16 else np.float32)
    b.run_stages(S_OFDM | S_CHEST, d.data_ptr(), stream())
    torch.cuda.synchronize()
    grid, ce = b.download(abi.BUF_GRID, np.float32), b.download(abi.BUF_CE, np.float32)
    met = b.download(abi.BUF_METRICS, np.float32).reshape(2, len(cfgs), 5)
    worst = dict(grid=0.0, ce=0.0, met=0.0)
    for a in range(2):
        for i, c in enumerate(cfgs):
            x = U.c128(iqs[a][i].astype(np.float64) / 32768.0) if sc16 else U.c128(iqs[a][i])
            rg = R.ofdm_rx(x, c.nof_prb)
            rc, rm = R.chest(rg, c.cell_id, c.nof_prb, c.nof_ports, c.sf)
            eg = rel_err(plane_part(b, abi.BUF_GRID, grid, a, i, 2 * rg.size), ri(rg))
            ec = rel_err(plane_part(b, abi.BUF_CE, ce, a, i, 2 * rc.size), ri(rc))
            em = float(np.max(np.abs(met[a, i] - rm) / np.abs(rm)))
            worst = dict(grid=max(worst["grid"], eg), ce=max(worst["ce"], ec), met=max(worst["met"], em))
            assert eg < TOL and ec < TOL, (a, i, c.nof_prb, c.nof_ports, eg, ec)
            assert em <= MET_TOL, (a, i, met[a, i].tolist(), rm.tolist())
    print("(a) front end: worst " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    b.close()


def front_inputs():
    """6, 15 and 100 PRB with 1 and 2 ports in one batch (the subframes' offsets differ, the plane stride is the
    batch's), each antenna with its own channel and noise at 20 dB"""
    cfgs = [plain_cfg(nprb, nof_ports=p, sf=1 + j, cell_id=20 + 7 * j + p) for j, nprb in enumerate((6, 15, 100)) for p in (1, 2)]
    iqs = [[U.ref_subframe(c, U.tb_bytes(i, c.tbs), U.channel(c, 60 + 2 * i + a), 20.0, 2 * i + a) for i, c in enumerate(cfgs)]
           for a in range(2)]
    return cfgs, iqs


@pytest.mark.parametrize("sc16", [False, True], ids=["fc32", "sc16"])
def test_front_end_per_antenna(sc16):
    cfgs, iqs = front_inputs()
    if sc16:
        iqs = [[abi.to_sc16(iq) for iq in per] for per in iqs]
    check_front(cfgs, iqs, sc16)


def test_front_end_256_subframes():
    """256 subframes of 6 PRB: the OFDM form that runs all 14 symbols of a subframe in one workgroup.  Eight reference
    subframes per antenna, dealt to the subframes in a different order per antenna and scaled per subframe, so every
    (antenna, subframe) holds samples of its own."""
    c = plain_cfg(6, nof_ports=2, sf=3, cell_id=33)
    base = [[U.ref_subframe(c, U.tb_bytes(40 + j, c.tbs), U.channel(c, 80 + 8 * a + j), 20.0, 8 * a + j) for j in range(8)]
            for a in range(2)]
    iqs = [[(base[a][(i + 3 * a) % 8] * np.float32(1.0 + i / 1024.0)).astype(np.float32) for i in range(256)] for a in range(2)]
    check_front([c] * 256, iqs)


# ------------------------------------------------------------------------------------------------ (b) demap alone
def test_demap_two_antennas_against_reference():
    """DEMAP alone (keep_llr) on uploaded reference grids and estimates of two antennas == pdsch_llr_rx at 1e-4 on the
    demap_cfgs() set (Qm 2 / 4 / 6 x TM1 / TM2, sf 0 and 5 at 6 PRB, cfi 1..3 at 6 and 100 PRB, a distributed
    allocation); the inputs keep the TM2 denominator >= 0.1 of its mean (pdsch_rx_ref.demap_rx_inputs)."""
    cfgs = tuple(demap_cfgs())
    ins = X.demap_rx_inputs(cfgs)
    b = abi.Batch([U.to_abi(c) for c in cfgs], keep_llr=True, n_rx=2)
    b.upload(abi.BUF_GRID, plane_buffer(b, abi.BUF_GRID, [[g[a] for g, _ in ins] for a in range(2)]))
    b.upload(abi.BUF_CE, plane_buffer(b, abi.BUF_CE, [[h[a] for _, h in ins] for a in range(2)]))
    b.run_stages(S_DEMAP, None, stream())
    llr = b.download(abi.BUF_LLR, np.float32)
    worst = 0.0
    for i, (c, (g32s, c32s)) in enumerate(zip(cfgs, ins)):
        want = X.pdsch_llr_rx(c, X.as_grids(c, g32s), X.as_ces(c, c32s))
        o = b.offset(abi.BUF_LLR, i)
        e = rel_err(llr[o:o + len(want)], want)
        worst = max(worst, e)
        assert e < TOL, (i, c.nof_prb, c.nof_ports, c.sf, c.cfi, c.Qm, e)
    print(f"(b) demap n_rx 2: worst llr rel_err {worst:.3e}")
    b.close()


# ------------------------------------------------------------------------------------------------ (c) fused == unfused
def tx_two(cfgs, seed):
    """the product transmitter once per antenna: the same TB through that antenna's flat channel, its own noise (20 dB)"""
    rng = np.random.default_rng(seed)
    tbs = [U.tb_bytes(seed + i, c.tbs) for i, c in enumerate(cfgs)]
    iqs = []
    for a in range(2):
        per = []
        for i, c in enumerate(cfgs):
            h = list(np.exp(2j * np.pi * rng.random(2)) * rng.uniform(0.6, 1.2, 2))
            per.append(abi.tx_subframe(c, tbs[i], h=h, snr_db=20.0, seed=1000 * seed + 2 * i + a))
        iqs.append(per)
    return tbs, iqs


def cfg_set(kind):
    mk = abi.sf_cfg
    if kind == "uniform_tm1":          # one modulation, new TBs, E <= N_v: direct groups
        return [mk(cell_id=11, nof_prb=15, nof_ports=1, sf_idx=1 + i, cfi=2, tbs=4008, Qm=4, rnti=0x50 + i) for i in range(3)]
    if kind == "uniform_tm2":
        return [mk(cell_id=12, nof_prb=15, nof_ports=2, sf_idx=1 + i, cfi=3, tbs=4008, Qm=6, rnti=0x60 + i) for i in range(3)]
    if kind == "mixed":                # Qm and TM differ between the lanes: unit_kind 0 (no code block repeats LLRs)
        return [mk(cell_id=13, nof_prb=6, nof_ports=1, sf_idx=1, cfi=1, tbs=1000, Qm=2, rnti=0x70),
                mk(cell_id=14, nof_prb=15, nof_ports=2, sf_idx=2, cfi=2, tbs=4008, Qm=4, rnti=0x71),
                mk(cell_id=15, nof_prb=15, nof_ports=1, sf_idx=3, cfi=3, tbs=4008, Qm=6, rnti=0x72),
                mk(cell_id=16, nof_prb=6, nof_ports=2, sf_idx=4, cfi=1, tbs=2024, Qm=6, rnti=0x73)]
    if kind == "repeat":               # code blocks that repeat LLRs (E > N_v): the single-LLR path, TM1 and TM2
        return [mk(cell_id=17, nof_prb=15, nof_ports=1 + i % 2, sf_idx=1 + i, cfi=1, tbs=104, Qm=2, rnti=0x80 + i) for i in range(4)]
    assert kind == "groups70"          # a full and a partial 64-lane group
    return [mk(cell_id=18, nof_prb=6, nof_ports=1, sf_idx=1 + i % 4, cfi=1, tbs=1000, Qm=2, rnti=0x90 + i) for i in range(70)]


def front_to_rm(cfgs, d_iqs, keep, retx=None):
    """OFDM | CHEST | DEMAP | RM on a two-antenna batch (then, retx = (cfgs, IQ): the same after a re-plan); returns the
    softbuffer arena's bits and the batch's group counts"""
    b = abi.Batch(cfgs, max_its=4, keep_llr=keep, n_rx=2)
    b.run_stages(S_OFDM | S_CHEST | S_DEMAP | S_RM, iq_planes(b, d_iqs).data_ptr(), stream())
    torch.cuda.synchronize()
    if retx is not None:
        plan = abi.Plan().build(retx[0])
        b.replan(plan, stream())
        b.run_stages(S_OFDM | S_CHEST | S_DEMAP | S_RM, iq_planes(b, retx[1]).data_ptr(), stream())
        torch.cuda.synchronize()
        plan.close()
    sb = b.download(abi.BUF_SB, np.uint32)
    counts = (b.n_groups, b.rm_direct_groups)
    b.close()
    return sb, counts


@pytest.mark.parametrize("kind", ["uniform_tm1", "uniform_tm2", "mixed", "retx", "repeat", "groups70"])
def test_fused_equals_unfused_two_antennas(kind):
    """The softbuffer after OFDM | CHEST | DEMAP | RM with the demap fused into rate de-matching == the one of the same
    run through demap_kernel and the LLR stream (keep_llr), bit for bit; then the full run with compact channel
    estimates decodes what the full run without them decodes."""
    retx = None
    if kind == "retx":                 # rv 0, then rv 2 with new_tb = 0: combining lanes, general groups
        cfgs = cfg_set("uniform_tm1")
        again = [abi.sf_cfg(cell_id=c.cell_id, nof_prb=15, nof_ports=1, sf_idx=c.sf_idx, cfi=2, tbs=c.tbs, Qm=4, rnti=c.rnti,
                            rv=2, new_tb=0) for c in cfgs]
        tbs, iqs = tx_two(cfgs, 7)
        retx = (again, [[abi.tx_subframe(c, tbs[i], h=[0.9 - 0.3j * a, 0.5], snr_db=20.0, seed=77 + 2 * i + a)
                         for i, c in enumerate(again)] for a in range(2)])
    else:
        cfgs = cfg_set(kind)
        tbs, iqs = tx_two(cfgs, 3 + len(kind))
    fused, counts = front_to_rm(cfgs, iqs, False, retx)
    unfused, _ = front_to_rm(cfgs, iqs, True, retx)
    n_groups, n_direct = counts
    if kind.startswith("uniform"):
        assert n_direct == n_groups > 0
    if kind == "retx":
        assert n_direct == 0
    if kind == "groups70":
        assert n_groups == 2
    assert fused.any() and np.array_equal(fused, unfused), int((fused != unfused).sum())
    # compact estimates (a batch with repeating code blocks keeps full ones): the same payloads and CRC verdicts
    res = []
    for compact in (False, True):
        b = abi.Batch(cfgs, max_its=4, compact_ce=compact, n_rx=2)
        b.run(iq_planes(b, iqs).data_ptr(), stream())
        torch.cuda.synchronize()
        res.append((b.download(abi.BUF_PAYLOAD, np.uint8), b.download(abi.BUF_TB_CRC, np.uint32)))
        if compact and kind != "repeat":
            with pytest.raises(RuntimeError, match="compact"):
                b.run_stages(S_DEMAP | S_RM | S_TDEC | S_TB, None, stream())
        for i in range(len(cfgs)):
            assert res[-1][1][i] == 1 and np.array_equal(b.payload(i, res[-1][0]), tbs[i]), (compact, i)
        b.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------ (d) n_rx = 1
def test_one_antenna_through_the_new_entry_point():
    """mi_dl_batch_create_rx(..., 1, ...) is mi_dl_batch_create: grid, ce, metrics, LLR and payload byte for byte, on the
    24 subframes of test_gpu_pdsch_ref.chain_inputs()"""
    cfgs, tbs, iqs, _ = chain_inputs()
    out = []
    for rx_entry in (False, True):
        b = abi.Batch([U.to_abi(c) for c in cfgs], max_its=4, keep_llr=True, rx_entry=rx_entry)
        assert b.n_rx == 1
        b.run(iq_planes(b, [iqs]).data_ptr(), stream())
        torch.cuda.synchronize()
        out.append([b.download(k, np.uint8) for k in (abi.BUF_GRID, abi.BUF_CE, abi.BUF_METRICS, abi.BUF_LLR, abi.BUF_PAYLOAD,
                                                      abi.BUF_TB_CRC)])
        for i in range(len(cfgs)):
            assert np.array_equal(b.payload(i, out[-1][4]), tbs[i]), i
        b.close()
    for x, y in zip(*out):
        assert len(x) == len(y) and np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ (e) diversity
def div_inputs():
    cases = [X.div_samples(name, seed) for name in X.DIV_CASES for seed in X.DIV_SEEDS]
    return [c for c, _, _ in cases], [t for _, t, _ in cases], [[U.f32c(s[a]) for _, _, s in cases] for a in range(2)]


def test_diversity_end_to_end():
    """The scenario test_pdsch_rx_ref.py pins (each antenna hears half of the band at 25 dB; 8 iterations, the default
    int16 decoder): a one-antenna batch fed either antenna's samples fails every TB CRC, the two-antenna batch decodes
    every transport block, its LLRs == pdsch_llr_rx of its own grids and estimates at 1e-4, and the host-IQ pipeline
    with two antennas decodes them too."""
    cfgs, tbs, iqs = div_inputs()
    acfgs = [U.to_abi(c) for c in cfgs]
    for a in range(2):
        b = abi.Batch(acfgs, max_its=8)
        b.run(iq_planes(b, [iqs[a]]).data_ptr(), stream())
        torch.cuda.synchronize()
        crc = b.download(abi.BUF_TB_CRC, np.uint32)
        assert not crc.any(), (a, crc.tolist())
        b.close()
    b = abi.Batch(acfgs, max_its=8, keep_llr=True, n_rx=2)
    b.run(iq_planes(b, iqs).data_ptr(), stream())
    torch.cuda.synchronize()
    pay, crc = b.download(abi.BUF_PAYLOAD, np.uint8), b.download(abi.BUF_TB_CRC, np.uint32)
    grid, ce, llr = (b.download(k, np.float32) for k in (abi.BUF_GRID, abi.BUF_CE, abi.BUF_LLR))
    worst = 0.0
    for i, c in enumerate(cfgs):
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs[i]), i
        n = R.NSYMB * c.W
        gs = X.as_grids(c, [plane_part(b, abi.BUF_GRID, grid, a, i, 2 * n) for a in range(2)])
        hs = X.as_ces(c, [plane_part(b, abi.BUF_CE, ce, a, i, 2 * n * c.nof_ports) for a in range(2)])
        want = X.pdsch_llr_rx(c, gs, hs)
        o = b.offset(abi.BUF_LLR, i)
        e = rel_err(llr[o:o + len(want)], want)
        worst = max(worst, e)
        assert e < TOL, (i, e)
    print(f"(e) diversity: worst llr rel_err {worst:.3e}")
    host_iq = iq_planes(b, iqs).cpu().numpy()
    b.close()
    pipe = abi.Pipe(acfgs, max_its=8, n_rx=2)
    hb = abi.HostBuffer(host_iq.nbytes)
    hb.array[:] = host_iq
    slot = pipe.submit(hb.ptr)
    pipe.wait(slot)
    pb = pipe.batch(slot)
    assert pb.n_rx == 2
    pay, crc = pb.download(abi.BUF_PAYLOAD, np.uint8), pb.download(abi.BUF_TB_CRC, np.uint32)
    for i in range(len(cfgs)):
        assert crc[i] == 1 and np.array_equal(pb.payload(i, pay), tbs[i]), i
    pipe.close()
    hb.close()


# ------------------------------------------------------------------------------------------------ (f) API edges
@pytest.mark.parametrize("n_rx", [0, 3])
def test_bad_antenna_count_is_refused(n_rx):
    with pytest.raises(RuntimeError, match="n_rx must be 1 or 2"):
        abi.Batch(cfg_set("mixed"), n_rx=n_rx, rx_entry=True)
    with pytest.raises(RuntimeError, match="n_rx must be 1 or 2"):
        abi.Pipe(cfg_set("mixed"), n_rx=n_rx)


def test_replan_two_antennas_to_a_larger_plan():
    """a two-antenna batch re-planned to more and wider subframes (every buffer and both plane strides grow) decodes
    what a fresh batch of that plan decodes"""
    small, large = cfg_set("mixed")[:1], cfg_set("mixed") + cfg_set("uniform_tm2")
    tbs_s, iqs_s = tx_two(small, 21)
    tbs_l, iqs_l = tx_two(large, 22)
    b = abi.Batch(small, max_its=4, n_rx=2)
    b.run(iq_planes(b, iqs_s).data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(b.payload(0), tbs_s[0])
    stride = b.rx_stride(abi.BUF_GRID)
    plan = abi.Plan().build(large)
    b.replan(plan, stream())
    assert b.rx_stride(abi.BUF_GRID) > stride and b.iq_rx_stride == b.iq_samples
    b.run(iq_planes(b, iqs_l).data_ptr(), stream())
    torch.cuda.synchronize()
    fresh = abi.Batch(large, max_its=4, n_rx=2)
    fresh.run(iq_planes(fresh, iqs_l).data_ptr(), stream())
    torch.cuda.synchronize()
    pay, crc = b.download(abi.BUF_PAYLOAD, np.uint8), b.download(abi.BUF_TB_CRC, np.uint32)
    assert np.array_equal(pay, fresh.download(abi.BUF_PAYLOAD, np.uint8))
    assert np.array_equal(crc, fresh.download(abi.BUF_TB_CRC, np.uint32))
    for i in range(len(large)):
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs_l[i]), i
    assert b.device_bytes >= fresh.device_bytes
    plan.close()
    fresh.close()
    b.close()


def test_control_channels_read_antenna_0():
    """mi_dl_ctrl_* on a two-antenna batch == on a one-antenna batch fed antenna 0's samples (soft bits bit for bit,
    the same CFI and DCI), whatever antenna 1 receives"""
    from test_gpu_ctrl import make_case
    built = [make_case(0, 25, 1, 1, 2, 0, None, 1, rnti=0x46), make_case(1, 25, 2, 2, 2, 1, 10.0, 2, rnti=0x47)]
    cfgs, iq0 = [x[0] for x in built], [x[2] for x in built]
    rng = np.random.default_rng(5)
    iq1 = [rng.standard_normal(len(iq)).astype(np.float32) for iq in iq0]
    got = []
    for n_rx in (1, 2):
        b = abi.Batch(cfgs, max_its=4, n_rx=n_rx)
        d = iq_planes(b, [iq0, iq1][:n_rx])
        b.run_stages(S_OFDM | S_CHEST, d.data_ptr(), stream())
        torch.cuda.synchronize()
        ctl = abi.Ctrl(b, phich_ng=2)
        ctl.run(stream())
        torch.cuda.synchronize()
        got.append((ctl.llr(), [ctl.result(s) for s in range(len(cfgs))]))
        ctl.close()
        b.close()
    assert np.array_equal(got[0][0], got[1][0])
    for s, (x, y) in enumerate(zip(got[0][1], got[1][1])):
        assert x[0] == y[0] == cfgs[s].cfi and x[1] is not None and y[1] is not None, s
        assert x[1][0] == y[1][0] and np.array_equal(x[1][1], y[1][1]) and x[1][2:] == y[1][2:], s
        assert np.array_equal(x[1][1], built[s][3]), s
