"""GPU: the DL receive kernels against tests/pdsch_ref.py, the independent float64 numpy reference (not the oracle).

Every expectation comes from pdsch_ref or from the transmitted bits.  Float stages are held to the 1e-4 of
BASELINE.json's north_star through helpers.rel_err (max |a - b| over the RMS of the reference); the channel metrics to
the 2e-3 of test_gpu_golden.py; decoder outputs are exact.  Each test prints the figure it asserts on.

(a) OFDM  (b) channel estimation  (c) gather + equalise + demap + descramble  (d) rate de-matching, HARQ, TB assembly
(e) the whole chain  (f) the turbo kernels at all 188 code-block sizes."""
import functools

import numpy as np
import pytest
import torch

import pdsch_ref as R
import pdsch_ref_util as U
from helpers import rel_err
from srsue_amd import abi
from test_gpu_parity import DECODERS
from test_gpu_tdec import MODES

pytestmark = pytest.mark.gpu

TOL = 1e-4
MET_TOL = 2e-3
S_OFDM, S_CHEST, S_DEMAP, S_RM, S_TDEC, S_TB = (1 << i for i in range(6))
BWS = (6, 15, 25, 50, 75, 100)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert torch.cuda.is_available()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ri(x):
    """complex array -> interleaved float64"""
    x = np.asarray(x).reshape(-1)
    return np.stack([x.real, x.imag], 1).reshape(-1)


def plain_cfg(nprb, **kw):
    """a subframe whose PDSCH does not matter (front-end stages only)"""
    return R.Cfg(nof_prb=nprb, tbs=104, Qm=2, **kw)


def flat_buffer(b, which, parts, scale, dtype=np.float32):
    """the batch's whole buffer `which` with parts[i] at subframe i's offset (scale: floats per offset unit)"""
    flat = np.zeros(abi.lib().mi_dl_batch_bytes(b.h, which) // np.dtype(dtype).itemsize, dtype)
    for i, p in enumerate(parts):
        o = scale * b.offset(which, i)
        flat[o:o + len(p)] = p
    return flat


def sf_part(b, which, buf, i, n, scale):
    o = scale * b.offset(which, i)
    return buf[o:o + n]


# ------------------------------------------------------------------------------------------------ (a) OFDM
def run_ofdm(cfgs, iqs, sc16=False):
    b = abi.Batch([U.to_abi(c) for c in cfgs], iq_sc16=sc16)
    flat = np.zeros(2 * b.iq_samples, np.int16 if sc16 else np.float32)
    for i, iq in enumerate(iqs):
        flat[2 * b.iq_offset(i):2 * b.iq_offset(i) + len(iq)] = iq
    d = torch.from_numpy(flat).cuda()
    b.run_stages(S_OFDM, d.data_ptr(), stream())
    torch.cuda.synchronize()
    g = b.download(abi.BUF_GRID, np.float32)
    out = [U.c128(sf_part(b, abi.BUF_GRID, g, i, 2 * R.NSYMB * c.W, 2)).reshape(R.NSYMB, c.W) for i, c in enumerate(cfgs)]
    b.close()
    return out


def test_ofdm_random_iq_all_bandwidths():
    """Complex Gaussian samples without any LTE structure, one subframe per bandwidth in one batch: the grid == numpy's
    FFT of the samples after each CP, on the bins the subcarriers map to."""
    rng = np.random.default_rng(1)
    cfgs = [plain_cfg(n) for n in BWS]
    iqs = [rng.standard_normal(2 * 15 * R.symbol_sz(n)).astype(np.float32) for n in BWS]
    worst = 0.0
    for c, iq, g in zip(cfgs, iqs, run_ofdm(cfgs, iqs)):
        e = rel_err(ri(g), ri(R.ofdm_rx(U.c128(iq), c.nof_prb)))
        worst = max(worst, e)
        assert e < TOL, c.nof_prb
    print(f"(a) ofdm random: worst rel_err {worst:.3e}")


def tone_subframe(nprb, bin_, amps):
    """one complex exponential on DFT bin `bin_` per symbol, amplitude amps[l], each symbol with its own cyclic prefix"""
    N = R.symbol_sz(nprb)
    out = []
    for l, cp in enumerate(R.cp_lens(N)):
        n = np.arange(-cp, N)
        out.append(amps[l] * np.exp(2j * np.pi * bin_ * n / N))
    return U.f32c(np.concatenate(out))


def test_ofdm_single_tones():
    """One tone per subframe on subcarrier 0, W/2 - 1, W/2 and W - 1, on the DC bin and on the first bin above the band, at
    every bandwidth (36 subframes, one batch), with a different complex amplitude in each symbol: the energy lands on
    exactly that (l, k) with the right complex value (a CP or symbol offset would turn its phase), or nowhere for the
    two out-of-band tones; everything else stays below 1e-4 of the tone."""
    rng = np.random.default_rng(2)
    cfgs, iqs, want = [], [], []
    for nprb in BWS:
        N, W = R.symbol_sz(nprb), 12 * nprb
        bins = R.bins(nprb)
        for k in (0, W // 2 - 1, W // 2, W - 1, "dc", "above"):
            b = 0 if k == "dc" else W // 2 + 1 if k == "above" else int(bins[k])
            amps = np.exp(2j * np.pi * rng.random(R.NSYMB)) * rng.uniform(0.5, 1.0, R.NSYMB)
            g = np.zeros((R.NSYMB, W), np.complex128)
            if not isinstance(k, str):
                g[:, k] = N * amps
            cfgs.append(plain_cfg(nprb)); iqs.append(tone_subframe(nprb, b, amps)); want.append((g, N * np.abs(amps).max()))
    # the bins the band does not use: DC and everything beyond +- W/2
    assert all(0 not in R.bins(n) and 6 * n + 1 not in R.bins(n) for n in BWS)
    worst = 0.0
    for i, (g, (w, peak)) in enumerate(zip(run_ofdm(cfgs, iqs), want)):
        e = float(np.max(np.abs(g - w)) / peak)
        worst = max(worst, e)
        assert e < TOL, (cfgs[i].nof_prb, i % 6)
    print(f"(a) ofdm tones: worst error / tone {worst:.3e}")


def test_ofdm_full_scale_sc16():
    """sc16 samples at the ends of the range (+32767 / -32768) mixed with random ones, all bandwidths: the grid == numpy's
    FFT of x / 32768."""
    rng = np.random.default_rng(3)
    cfgs = [plain_cfg(n) for n in BWS]
    iqs = []
    for n in BWS:
        x = rng.integers(-32768, 32768, 2 * 15 * R.symbol_sz(n))
        ext = rng.random(len(x)) < 0.5
        x[ext] = np.where(rng.random(int(ext.sum())) < 0.5, 32767, -32768)
        iqs.append(x.astype(np.int16))
    worst = 0.0
    for c, iq, g in zip(cfgs, iqs, run_ofdm(cfgs, iqs, sc16=True)):
        e = rel_err(ri(g), ri(R.ofdm_rx(U.c128(iq.astype(np.float64) / 32768.0), c.nof_prb)))
        worst = max(worst, e)
        assert e < TOL, c.nof_prb
    print(f"(a) ofdm sc16: worst rel_err {worst:.3e}")


# ------------------------------------------------------------------------------------------------ (b) channel estimation
CHEST_CFGS = [plain_cfg(nprb, nof_ports=ports, sf=sf, cell_id=6 * ((3 * i + nprb + sf) % 80) + i)   # id mod 6 = i
              for nprb in (6, 15, 100) for ports in (1, 2) for sf in (0, 9) for i in range(6)]


@pytest.mark.parametrize("snr", [None, 20.0], ids=["noiseless", "20dB"])
def test_chest_selective_channel(snr):
    """CHEST alone on uploaded reference grids: random data and the cell's CRS through a three-tap channel (delays inside
    the CP) times a per-symbol phase ramp, so smoothing, frequency interpolation, edge extrapolation and time
    interpolation all see a channel that is not flat.  ce == pdsch_ref.chest at 1e-4 over 1.4 / 3 / 20 MHz, 1 / 2 ports,
    sf 0 / 9 and cell ids of every id mod 6; the five metrics at 2e-3 on the noisy run (without noise the noise metric
    is a cancellation)."""
    cfgs = CHEST_CFGS
    assert sorted({c.cell_id % 6 for c in cfgs}) == list(range(6))
    grids = [U.f32c(U.rx_grid(U.filled_grid(c, i), U.channel(c, i), snr, i)) for i, c in enumerate(cfgs)]
    b = abi.Batch([U.to_abi(c) for c in cfgs])
    b.upload(abi.BUF_GRID, flat_buffer(b, abi.BUF_GRID, grids, 2))
    b.run_stages(S_CHEST, None, stream())
    ce = b.download(abi.BUF_CE, np.float32)
    met = b.download(abi.BUF_METRICS, np.float32).reshape(-1, 5)
    worst, worst_m = 0.0, 0.0
    for i, c in enumerate(cfgs):
        rce, rmet = R.chest(U.c128(grids[i]).reshape(R.NSYMB, c.W), c.cell_id, c.nof_prb, c.nof_ports, c.sf)
        e = rel_err(sf_part(b, abi.BUF_CE, ce, i, 2 * rce.size, 2), ri(rce))
        worst = max(worst, e)
        assert e < TOL, (i, c.nof_prb, c.nof_ports, c.sf, c.cell_id)
        if snr is not None:
            em = float(np.max(np.abs(met[i] - rmet) / np.abs(rmet)))
            worst_m = max(worst_m, em)
            assert em <= MET_TOL, (i, met[i].tolist(), rmet.tolist())
    print(f"(b) chest {snr}: worst ce rel_err {worst:.3e}, worst metric error {worst_m:.3e}")
    b.close()


# ------------------------------------------------------------------------------------------------ (c) demap
def demap_cfgs():
    out = []
    for j, (Qm, ports) in enumerate((q, p) for q in (2, 4, 6) for p in (1, 2)):
        out.append(R.Cfg(cell_id=30 + j, nof_prb=15, nof_ports=ports, sf=1, cfi=2, tbs=104, Qm=Qm, rnti=0x100 + j))
    for sf in (0, 5):                                           # at 6 PRB the PBCH / sync holes span the band
        for ports in (1, 2):
            out.append(R.Cfg(cell_id=100 + sf + ports, nof_prb=6, nof_ports=ports, sf=sf, cfi=1, tbs=104, Qm=4))
    for nprb in (6, 100):
        for cfi in (1, 2, 3):
            out.append(R.Cfg(cell_id=200 + cfi, nof_prb=nprb, nof_ports=1 + cfi % 2, sf=3, cfi=cfi, tbs=104, Qm=6))
    dist = np.random.default_rng(4).random((2, 25)) < 0.5
    dist[0, :2], dist[1, :2] = (True, False), (False, True)
    out.append(R.Cfg(cell_id=17, nof_prb=25, nof_ports=2, sf=7, cfi=1, tbs=104, Qm=4, prb_slots=dist))
    assert {c.cell_id % 3 for c in out if c.tm == 1} == {0, 1, 2} == {c.cell_id % 3 for c in out if c.tm == 2}
    return out


def test_demap_reference_grid_and_ce():
    """DEMAP alone (keep_llr) on uploaded reference grid + channel: RE gather, TM1 MMSE / TM2 equaliser, max-log demapper
    and descrambling == pdsch_ref at 1e-4 for Qm 2 / 4 / 6 x TM1 / TM2, sf 0 and 5 at 6 PRB, cfi 1..3 at 6 and 100 PRB, a
    distributed allocation and cell ids of every id mod 3."""
    cfgs = demap_cfgs()
    grids, ces, want = [], [], []
    for i, c in enumerate(cfgs):
        H = U.channel(c, 20 + i)
        if c.tm == 2:      # the TM2 equaliser divides by |h00|^2 + |h11|^2: keep it away from a null
            m = c.re_mask()
            hh = np.abs(H[0][m][0::2]) ** 2 + np.abs(H[1][m][1::2]) ** 2
            assert hh.min() >= 0.1 * hh.mean(), (i, hh.min() / hh.mean())
        g32, c32 = U.f32c(U.rx_grid(U.pdsch_symbol_grid(c, i), H, 25.0, i)), U.f32c(H)
        grids.append(g32); ces.append(c32)
        want.append(R.pdsch_llr(c, U.c128(g32).reshape(R.NSYMB, c.W), U.c128(c32).reshape(c.nof_ports, R.NSYMB, c.W)))
    b = abi.Batch([U.to_abi(c) for c in cfgs], keep_llr=True)
    b.upload(abi.BUF_GRID, flat_buffer(b, abi.BUF_GRID, grids, 2))
    b.upload(abi.BUF_CE, flat_buffer(b, abi.BUF_CE, ces, 2))
    b.run_stages(S_DEMAP, None, stream())
    llr = b.download(abi.BUF_LLR, np.float32)
    worst = 0.0
    for i, c in enumerate(cfgs):
        assert abi.pdsch_G(U.to_abi(c)) == len(want[i])
        e = rel_err(sf_part(b, abi.BUF_LLR, llr, i, len(want[i]), 1), want[i])
        worst = max(worst, e)
        assert e < TOL, (i, c.nof_prb, c.nof_ports, c.sf, c.cfi, c.Qm)
    print(f"(c) demap: worst llr rel_err {worst:.3e}")
    b.close()


# ------------------------------------------------------------------------------------------------ (d) RM, HARQ, TB
N_REP = 70     # a full and a partial 64-lane group; the packed decoder pairs them


@pytest.mark.parametrize("i16,sched", DECODERS)
@pytest.mark.parametrize("name", list(U.DECODE_CASES))
def test_decode_reference_llrs(name, i16, sched):
    """RM | TDEC | TB on uploaded reference LLRs of 70 subframes with distinct RNTI and TB: payload == the transmitted TB
    and TB CRC == 1, in every decoder."""
    cfgs, tbs, llrs = U.decode_case(name, N_REP)
    b = abi.Batch([U.to_abi(c) for c in cfgs], max_its=4, tdec_i16=i16, sched=sched)
    b.upload(abi.BUF_LLR, flat_buffer(b, abi.BUF_LLR, llrs, 1))
    b.run_stages(S_RM | S_TDEC | S_TB, None, stream())
    pay = b.download(abi.BUF_PAYLOAD, np.uint8)
    crc = b.download(abi.BUF_TB_CRC, np.uint32)
    for i in range(N_REP):
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs[i]), i
    b.close()


@pytest.mark.parametrize("i16,sched", DECODERS)
@pytest.mark.parametrize("name", list(U.HARQ_CASES))
def test_harq_sequence_reference_llrs(name, i16, sched):
    """rv 0, 2, 3, 1 of one TB combined in the batch's softbuffer (the same grant re-planned with the next rv) at the
    operating point test_pdsch_ref.py fixes: the TB CRC fails with need - 1 transmissions and passes with need, where
    the payload is the transmitted TB.  need = 2, 3 and 4: the last case puts every k0 on the GPU."""
    harq_sequence(name, i16, sched, fused=False)


@pytest.mark.parametrize("i16,sched", DECODERS)
@pytest.mark.parametrize("name", list(U.HARQ_CASES))
def test_harq_sequence_fused_from_reference_grid(name, i16, sched):
    """The same sequences on the default path: each transmission uploaded as reference grid + channel, demap fused into
    rate de-matching (no LLR stream), retransmissions combining (new_tb = 0) -- fail and pass at the same transmissions."""
    harq_sequence(name, i16, sched, fused=True)


def harq_sequence(name, i16, sched, fused):
    cfgs, tb, grids, ces, llrs, need = U.harq_case(name)
    b = abi.Batch([U.to_abi(cfgs[0], new_tb=1)], max_its=4, tdec_i16=i16, sched=sched)
    plan = abi.Plan()
    for t in range(need):
        if t:
            plan.build([U.to_abi(cfgs[t], new_tb=0)])
            b.replan(plan, stream())
        if fused:
            b.upload(abi.BUF_GRID, flat_buffer(b, abi.BUF_GRID, [grids[t]], 2))
            b.upload(abi.BUF_CE, flat_buffer(b, abi.BUF_CE, [ces[t]], 2))
            b.run_stages(S_DEMAP | S_RM | S_TDEC | S_TB, None, stream())
        else:
            b.upload(abi.BUF_LLR, flat_buffer(b, abi.BUF_LLR, [llrs[t]], 1))
            b.run_stages(S_RM | S_TDEC | S_TB, None, stream())
        crc = b.download(abi.BUF_TB_CRC, np.uint32)
        assert bool(crc[0]) == (t == need - 1), t
    assert np.array_equal(b.payload(0), tb)
    b.close()
    plan.close()


@functools.lru_cache(None)
def fused_inputs():
    """three subframes of every DECODE_CASES entry as reference grid + channel (float32) and their TBs"""
    cfgs, tbs, grids, ces = [], [], [], []
    for name, (kw, snr) in U.DECODE_CASES.items():
        for i in range(3):
            c = R.Cfg(rnti=0x61 + i, **kw)
            tb = U.tb_bytes(300 + i + len(name), c.tbs)
            H = U.channel(c, i, taps=(1.0, 0.2, 0.1))
            cfgs.append(c); tbs.append(tb); ces.append(U.f32c(H))
            grids.append(U.f32c(U.rx_grid(R.tx_grid(c, tb, U.qpp()), H, snr + 3.0, i)))
    return cfgs, tbs, grids, ces


@pytest.mark.parametrize("i16,sched", DECODERS)
def test_decode_fused_from_reference_grid(i16, sched):
    """The default path (demap fused into rate de-matching, no LLR stream) from uploaded reference grid + channel, the
    five cases mixed in one batch: payload == the transmitted TB."""
    cfgs, tbs, grids, ces = fused_inputs()
    b = abi.Batch([U.to_abi(c) for c in cfgs], max_its=4, tdec_i16=i16, sched=sched)
    b.upload(abi.BUF_GRID, flat_buffer(b, abi.BUF_GRID, grids, 2))
    b.upload(abi.BUF_CE, flat_buffer(b, abi.BUF_CE, ces, 2))
    b.run_stages(S_DEMAP | S_RM | S_TDEC | S_TB, None, stream())
    pay = b.download(abi.BUF_PAYLOAD, np.uint8)
    crc = b.download(abi.BUF_TB_CRC, np.uint32)
    for i in range(len(cfgs)):
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs[i]), i
    b.close()


# ------------------------------------------------------------------------------------------------ (e) whole chain
@functools.lru_cache(None)
def chain_inputs(rate64=0.33):
    """reference transmit of 24 subframes (six bandwidths x TM1 / TM2 x sf 0 / 5) through the selective channel at 30 dB,
    and the reference receiver's grid / ce / llr of the float32 samples.  Code rate 0.4, and rate64 for 64QAM: at
    0.33 those code blocks repeat part of the circular buffer (E > N_v)."""
    cfgs, tbs, iqs, refs = [], [], [], []
    for j, nprb in enumerate(BWS):
        for ports in (1, 2):
            for sf in (0, 5):
                Qm = (2, 4, 6)[(j + ports + sf) % 3]
                c0 = R.Cfg(cell_id=40 * j + 7 * ports + sf, nof_prb=nprb, nof_ports=ports, sf=sf, cfi=1 + j % 3, Qm=Qm)
                tbs_bits = max(16, int(c0.G * (rate64 if Qm == 6 else 0.4)) // 8 * 8)
                c = R.Cfg(cell_id=c0.cell_id, nof_prb=nprb, nof_ports=ports, sf=sf, cfi=c0.cfi, Qm=Qm, tbs=tbs_bits,
                          rnti=0x200 + len(cfgs))
                tb = U.tb_bytes(500 + len(cfgs), c.tbs)
                iq = U.ref_subframe(c, tb, U.channel(c, len(cfgs), taps=(1.0, 0.3, 0.15)), 30.0, len(cfgs))
                cfgs.append(c); tbs.append(tb); iqs.append(iq); refs.append(U.ref_front(c, iq))
    return cfgs, tbs, iqs, refs


def run_chain(cfgs, iqs, **kw):
    b = abi.Batch([U.to_abi(c) for c in cfgs], max_its=4, **kw)
    flat = np.zeros(2 * b.iq_samples, np.float32)
    for i, iq in enumerate(iqs):
        flat[2 * b.iq_offset(i):2 * b.iq_offset(i) + len(iq)] = iq
    d = torch.from_numpy(flat).cuda()
    b.run(d.data_ptr(), stream())
    torch.cuda.synchronize()
    return b


def test_whole_chain_against_reference():
    """A full run on reference subframes: grid, ce and LLR == the reference receiver at 1e-4, payload == the TB."""
    cfgs, tbs, iqs, refs = chain_inputs()
    b = run_chain(cfgs, iqs, keep_llr=True)
    grid, ce, llr = (b.download(k, np.float32) for k in (abi.BUF_GRID, abi.BUF_CE, abi.BUF_LLR))
    pay = b.download(abi.BUF_PAYLOAD, np.uint8)
    crc = b.download(abi.BUF_TB_CRC, np.uint32)
    worst = dict(grid=0.0, ce=0.0, llr=0.0)
    for i, c in enumerate(cfgs):
        rg, rc, _, rl = refs[i]
        for key, which, buf, ref, scale in (("grid", abi.BUF_GRID, grid, ri(rg), 2), ("ce", abi.BUF_CE, ce, ri(rc), 2),
                                            ("llr", abi.BUF_LLR, llr, rl, 1)):
            e = rel_err(sf_part(b, which, buf, i, len(ref), scale), ref)
            worst[key] = max(worst[key], e)
            assert e < TOL, (key, i, c.nof_prb, c.nof_ports, c.sf, c.Qm)
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs[i]), i
    print("(e) chain: worst rel_err " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    b.close()


@pytest.mark.parametrize("i16,sched", DECODERS)
def test_whole_chain_compact_ce_decodes(i16, sched):
    """The same 24 cells, bandwidths, ports and subframes through the default run with compact channel estimates (4 pilot
    rows per port, time interpolation inside the fused demap): payload == the TB in every decoder.  A batch runs
    compact only when no code block repeats LLRs (E <= N_v = 3 (K + 4) - 2 F for all of them; otherwise it
    falls back to full estimates), so 64QAM is sent at rate 0.45 here and the precondition is asserted from the
    reference.  That the estimates were compact is asserted too: a DEMAP run without CHEST on them is rejected
    (include/mi_dl.h, MI_DL_FLAG_CE_COMPACT)."""
    cfgs, tbs, iqs, _ = chain_inputs(rate64=0.45)
    for c in cfgs:
        sg = R.segment(c.tbs + 24)
        for r in range(sg["C"]):
            K, F = (sg["Km"] if r < sg["Cm"] else sg["Kp"]), (sg["F"] if r == 0 else 0)
            assert R.rm_E(c.G, sg["C"], c.Qm, c.NL, r) <= 3 * (K + 4) - 2 * F, (c.nof_prb, c.Qm, r)
    b = run_chain(cfgs, iqs, compact_ce=True, tdec_i16=i16, sched=sched)
    pay = b.download(abi.BUF_PAYLOAD, np.uint8)
    crc = b.download(abi.BUF_TB_CRC, np.uint32)
    for i in range(len(cfgs)):
        assert crc[i] == 1 and np.array_equal(b.payload(i, pay), tbs[i]), i
    with pytest.raises(RuntimeError, match="compact"):
        b.run_stages(S_DEMAP | S_RM | S_TDEC | S_TB, None, stream())
    b.close()


# ------------------------------------------------------------------------------------------------ (f) all 188 K
ALL_K = [int(k) for k in R.CB_SIZES]
N_CHUNK = 8
CHUNKS = [ALL_K[i::N_CHUNK] for i in range(N_CHUNK)]      # every chunk spans 40 .. 6144
N_CB = U.N_CB
blocks, oracle_decisions = U.blocks, U.oracle_decisions      # cached for the module: once per K, point and arithmetic


def gpu_decode(K, llr, i16, sched, **kw):
    tb = abi.TdecBatch(K, len(llr), tdec_i16=i16, sched=sched, **kw)
    d = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    tb.run(d.data_ptr(), stream())
    out = tb.results()
    tb.close()
    return out


@pytest.mark.parametrize("i16,sched", MODES)
@pytest.mark.parametrize("chunk", range(N_CHUNK))
def test_all_code_block_sizes_easy_point(chunk, i16, sched):
    """70 CRC24A-carrying blocks per K from the reference encoder at an Eb/N0 where both oracle decoders recover every
    block: decoded bits == the transmitted ones, iterations and CRC verdicts == the oracle of the same arithmetic."""
    for K in CHUNKS[chunk]:
        bits, llr = blocks(K, True)
        obits, oits, ook = oracle_decisions(K, True, i16)
        got, its, ok = gpu_decode(K, llr, i16, sched, max_its=6, early_stop=True, crc24a=True)
        assert np.array_equal(got, bits), K
        assert np.array_equal(its, oits) and np.array_equal(ok.astype(bool), ook), K
        assert ook.all() and np.array_equal(obits, bits), K


@pytest.mark.parametrize("i16,sched", MODES)
@pytest.mark.parametrize("chunk", range(N_CHUNK))
def test_all_code_block_sizes_waterfall_point(chunk, i16, sched):
    """The same sizes where 4 iterations leave residual errors in part of the blocks: decisions bit-identical to the
    oracle of the same arithmetic (a K-dependent span, window or tail error shows in the unconverged blocks)."""
    wrong = 0
    for K in CHUNKS[chunk]:
        bits, llr = blocks(K, False)
        obits, _, _ = oracle_decisions(K, False, i16)
        got, its, _ = gpu_decode(K, llr, i16, sched, max_its=4, early_stop=False)
        assert np.array_equal(got, obits), K
        assert np.all(its == 4), K
        wrong += int((obits != bits).any(1).sum())
    assert wrong > len(CHUNKS[chunk])          # the point is in the waterfall
