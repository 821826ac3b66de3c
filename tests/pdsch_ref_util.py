"""Bridges between tests/pdsch_ref.py (numpy only) and the code under test: configuration conversion, the transcribed
QPP table, the selective test channel, reference subframes.  Shared by test_pdsch_ref.py and test_gpu_pdsch_ref.py."""
import concurrent.futures
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
import pdsch_ref as R
from srsue_amd import abi


@functools.lru_cache(None)
def qpp():
    """K -> (f1, f2), 36.212 Table 5.1.3-3 as transcribed in oracle/o_common.c (spot values pinned by test_oracle.py)"""
    out = {}
    for K in R.CB_SIZES:
        f1, f2 = C.c_uint32(), C.c_uint32()
        assert O.lib().or_qpp_f(int(K), C.byref(f1), C.byref(f2)) == 0
        out[int(K)] = (f1.value, f2.value)
    return out


def prb_mask_u8(cfg):
    """the C structs' prb_mask: 0 / 1 when both slots agree, else bit s = used in slot s"""
    s = cfg.prb_slots.astype(np.uint8)
    m = np.zeros(O.NRB_MAX, np.uint8)
    m[:cfg.nof_prb] = s[0] if np.array_equal(s[0], s[1]) else s[0] | (s[1] << 1)
    return m


def to_abi(cfg, new_tb=1):
    return abi.sf_cfg(cell_id=cfg.cell_id, nof_prb=cfg.nof_prb, nof_ports=cfg.nof_ports, sf_idx=cfg.sf, cfi=cfg.cfi,
                      tm=cfg.tm, rnti=cfg.rnti, rv=cfg.rv, tbs=cfg.tbs, Qm=cfg.Qm, new_tb=new_tb,
                      prb=prb_mask_u8(cfg)[:cfg.nof_prb], nl_td=cfg.NL if cfg.tm == 2 else 2)


def to_otx(cfg, h, snr_db=300.0):
    return O.tx_cfg(O.make_cell(cfg.cell_id, cfg.nof_prb, cfg.nof_ports), sf_idx=cfg.sf, cfi=cfg.cfi, rv=cfg.rv,
                    rnti=cfg.rnti, tm=cfg.tm, tbs=cfg.tbs, qm=cfg.Qm, prb=prb_mask_u8(cfg)[:cfg.nof_prb],
                    snr_db=snr_db, h=h, nl_td=cfg.NL if cfg.tm == 2 else 2)


def tb_bytes(seed, tbs):
    return np.random.default_rng(0x7B000 + seed).integers(0, 256, tbs // 8).astype(np.uint8)


def channel(cfg, seed=0, ramp=0.04, taps=(1.0, 0.45, 0.25)):
    """H[port, l, k]: three taps per port (magnitudes `taps`, random phases) with delays 0, N/128 and 3N/128 samples
    (inside the shortest CP, 9N/128) times a phase ramp of `ramp` rad per symbol -- known exactly, selective in
    frequency and varying in time; unit mean power."""
    rng = np.random.default_rng(0xC4A0 + seed)
    N = R.symbol_sz(cfg.nof_prb)
    f = R.bins(cfg.nof_prb).astype(np.float64)
    f = np.where(f >= N / 2, f - N, f) / N                        # cycles per sample
    H = np.zeros((cfg.nof_ports, R.NSYMB, cfg.W), np.complex128)
    for p in range(cfg.nof_ports):
        amp = np.array(taps) * np.exp(2j * np.pi * rng.random(3))
        resp = sum(a * np.exp(-2j * np.pi * f * d * N / 128) for a, d in zip(amp, (0, 1, 3)))
        H[p] = resp[None, :] * np.exp(1j * ramp * (p + 1) * np.arange(R.NSYMB))[:, None]
    return H / np.sqrt(np.sum(np.square(taps)))


def f32c(x):
    """complex array -> interleaved float32 (the code under test's wire format)"""
    x = np.asarray(x, np.complex128).reshape(-1)
    return np.stack([x.real, x.imag], 1).reshape(-1).astype(np.float32)


def c128(x):
    """interleaved float32 -> complex128"""
    x = np.asarray(x, np.float64).reshape(-1, 2)
    return x[:, 0] + 1j * x[:, 1]


def ref_subframe(cfg, tb, H=None, snr_db=None, seed=0):
    """reference transmit of one subframe: interleaved float32 samples (what every receiver under test is fed)"""
    grids = R.tx_grid(cfg, tb, qpp())
    return f32c(R.ofdm_tx(grids, H, snr_db, np.random.default_rng(0xA0150 + seed)))


def ref_front(cfg, iq32):
    """reference receive front end on the float32 samples: (grid, ce, metrics, llr) in float64"""
    return R.rx_front(cfg, c128(iq32))


def rx_grid(grids, H, snr_db=None, seed=0):
    """the received grid of per-port transmit grids through H[port, l, k], formed in the frequency domain (what a
    perfect OFDM receiver yields, up to its sqrt(N) gain): sum_p H_p X_p + AWGN of variance 10^(-snr / 10) per RE"""
    y = (grids * H).sum(0)
    if snr_db is not None:
        rng = np.random.default_rng(0x6A1D + seed)
        y = y + np.sqrt(10.0 ** (-snr_db / 10.0) / 2.0) * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    return y


def filled_grid(cfg, seed=0):
    """per-port grids [P, 14, W] of random QPSK on every RE (no transport block), the cell's CRS on top and nothing on
    the other port's CRS positions: all the channel estimator looks at"""
    rng = np.random.default_rng(0xF111 + seed)
    g = R.modulate(rng.integers(0, 2, 2 * cfg.nof_ports * R.NSYMB * cfg.W), 2).reshape(cfg.nof_ports, R.NSYMB, cfg.W)
    if cfg.nof_ports == 2:
        g = g / np.sqrt(2)
    for l in (0, 4, 7, 11):
        for p in range(cfg.nof_ports):
            r, k = R.crs(cfg.cell_id, 2 * cfg.sf + l // 7, l % 7, p, cfg.nof_prb)
            g[:, l, k] = 0
            g[p, l, k] = r
    return g


def pdsch_symbol_grid(cfg, seed=0):
    """per-port grids holding random modulation symbols of cfg.Qm on the PDSCH REs only (TM2: SFBC pairs): all the
    gather / equalise / demap stage looks at"""
    rng = np.random.default_rng(0x5B0 + seed)
    mask = cfg.re_mask()
    x = R.modulate(rng.integers(0, 2, int(mask.sum()) * cfg.Qm), cfg.Qm)
    g = np.zeros((cfg.nof_ports, R.NSYMB, cfg.W), np.complex128)
    if cfg.tm == 2:
        y = R.sfbc(x)
        g[0][mask], g[1][mask] = y[0], y[1]
    else:
        g[0][mask] = x
    return g


# ---- raw code blocks of every size (test_gpu_pdsch_ref.py part f): BPSK / AWGN LLRs of reference-encoded blocks
def ebno_easy(K):
    """Eb/N0 (dB) at which both oracle decoders recover every block of size K within 6 iterations (chosen on the CPU
    per K range, test_pdsch_ref.py::test_code_block_operating_points keeps it true)"""
    return 7.0 if K < 128 else 5.0 if K < 512 else 3.5 if K < 2048 else 2.5


def ebno_waterfall(K):
    """Eb/N0 (dB) that leaves residual errors after 4 iterations in part of the 70 blocks"""
    return 1.5 if K < 128 else 1.0 if K < 2048 else 0.85


def code_blocks(K, n, ebno_db, crc24a, seed=0):
    """n blocks of size K from the reference encoder as BPSK / AWGN LLRs (LLR > 0: bit 1) in the decoder's triplet
    order: (bits[n, K], llr[n, 3 (K + 4)] float32).  crc24a: the last 24 bits are the CRC24A of the first K - 24."""
    rng = np.random.default_rng(1000 * K + seed)
    bits = rng.integers(0, 2, (n, K)).astype(np.uint8)
    if crc24a:
        bits[:, K - 24:] = R.crc_many(bits[:, :K - 24], R.CRC24A)
    d = R.turbo_encode_many(bits, *qpp()[K]).transpose(0, 2, 1).reshape(n, -1)
    s2 = 1.0 / (2 * (K / (3.0 * K + 12)) * 10 ** (ebno_db / 10))
    y = (2.0 * d - 1.0) + rng.normal(0, np.sqrt(s2), d.shape)
    return bits, (2.0 * y / s2).astype(np.float32)


N_CB = 70     # blocks per size: a full and a partial 64-lane group


@functools.lru_cache(None)
def blocks(K, easy):
    """the N_CB blocks of size K at the easy (CRC24A-carrying) or the waterfall point"""
    return code_blocks(K, N_CB, ebno_easy(K) if easy else ebno_waterfall(K), crc24a=easy)


@functools.lru_cache(None)
def oracle_decisions(K, easy, i16):
    """(bits[n, K], iterations[n], crc ok[n]) of the oracle decoder of one arithmetic on blocks(K, easy): 6 iterations
    with CRC24A early stop at the easy point, 4 iterations without early stop at the waterfall point.  int16: the
    SSE implementation (bit-identical to or_decode_cb16, test_oracle.py) over 8 threads; float: 8 decoders in threads."""
    _, llr = blocks(K, easy)
    its_max, stop = (6, True) if easy else (4, False)
    bits, its, ok = np.zeros((N_CB, K), np.uint8), np.zeros(N_CB, np.uint32), np.zeros(N_CB, np.uint8)
    if i16:
        assert O.lib().or_simd_decode_batch(llr.reshape(-1), llr.shape[1], N_CB, K, its_max, int(stop), int(easy),
                                            bits.reshape(-1), its, ok, 8) == 0
        return bits, its, ok.astype(bool)

    def work(j):
        td = O.Tdec(O.TDEC_GEN)
        for i in range(j, N_CB, 8):
            bits[i], its[i], ok[i] = td.decode_cb(llr[i], K, max_its=its_max, early_stop=stop, crc24a=easy)
            assert 1 <= its[i] <= its_max          # or_decode_cb returns -1 on a bad K
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        list(ex.map(work, range(8)))
    return bits, its, ok.astype(bool)


# ---- the rate de-matching / HARQ / TB assembly cases (test_gpu_pdsch_ref.py part d), shared by the emulated-kernel and the GPU tests
DECODE_CASES = {
    # name: (Cfg arguments, per-RE SNR in dB of the symbol-level AWGN the reference LLRs are formed at)
    "tbs16_K40_wraps": (dict(cell_id=3, nof_prb=6, sf=1, tbs=16, Qm=2, rv=3), 6.0),       # E = 1656 >> N_cb = 192
    "tbs512_F8": (dict(cell_id=4, nof_prb=6, sf=2, tbs=512, Qm=2), 6.0),                   # C = 1, K = 544, F = 8
    "tbs7000_KmKp_F32": (dict(cell_id=11, nof_prb=25, sf=4, tbs=7000, Qm=4, rv=2), 14.0),  # C = 2, K- / K+, F = 32
    "punctured_64qam": (dict(cell_id=301, nof_prb=6, sf=1, tbs=4392, Qm=6), 30.0),         # rate 0.89, K = 4416
    "tm2_NL2": (dict(cell_id=7, nof_prb=25, nof_ports=2, sf=3, tbs=7000, Qm=4, cfi=2, rv=1), 14.0),
}
# HARQ: redundancy versions 0, 2, 3, 1 of one TB at an SNR where decoding needs more than one transmission
HARQ_RVS = (0, 2, 3, 1)
HARQ_CASES = {
    # name: (Cfg arguments, SNR, number of transmissions the reference decoder needs)
    "punctured_64qam": (dict(cell_id=301, nof_prb=6, sf=1, tbs=4392, Qm=6), 14.5, 2),
    "tbs512_three_tx": (dict(cell_id=4, nof_prb=6, sf=2, tbs=512, Qm=2), -5.2, 3),
    "tbs512_four_tx": (dict(cell_id=4, nof_prb=6, sf=2, tbs=512, Qm=2), -6.3, 4),          # all four k0 values
}


def ref_llr_awgn(cfg, tb, snr_db, seed):
    """Reference soft bits of one transmission without the OFDM / channel-estimation stages: the reference's coded,
    scrambled, modulated symbols plus AWGN at snr_db per RE, demapped and descrambled by the reference (float32)."""
    G = cfg.G
    f = R.dlsch_encode(cfg.tbs, R.bytes_to_bits(tb)[:cfg.tbs], G, cfg.Qm, cfg.NL, cfg.rv, qpp())
    ci = R.pdsch_c_init(cfg.rnti, cfg.sf, cfg.cell_id)
    x = R.modulate(R.scramble(f, ci), cfg.Qm)
    rng = np.random.default_rng(0x11A0 + seed)
    s = np.sqrt(10.0 ** (-snr_db / 10.0) / 2.0)
    x = x + s * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    return R.descramble(R.demap(x, cfg.Qm), ci).astype(np.float32)


@functools.lru_cache(None)
def decode_case(name, n=1):
    """n subframes of DECODE_CASES[name] with distinct RNTI and TB: (cfgs, tbs, llrs)"""
    kw, snr = DECODE_CASES[name]
    cfgs = [R.Cfg(rnti=0x46 + 3 * i, **kw) for i in range(n)]
    tbs = [tb_bytes(17 * i + len(name), c.tbs) for i, c in enumerate(cfgs)]
    return cfgs, tbs, [ref_llr_awgn(c, t, snr, i) for i, (c, t) in enumerate(zip(cfgs, tbs))]


@functools.lru_cache(None)
def harq_case(name):
    """The transmissions of one TB as reference grid + channel (float32) and the reference LLRs of exactly those arrays,
    so the LLR-upload path and the fused path see the same soft bits:
    (cfgs per transmission, tb, grids, ces, llrs, transmissions needed).  The channel has unit magnitude (one tap, a
    phase per port and a phase ramp over the symbols), so the operating point is the AWGN one."""
    kw, snr, need = HARQ_CASES[name]
    cfgs = [R.Cfg(rv=rv, **kw) for rv in HARQ_RVS]
    tb = tb_bytes(99 + len(name), cfgs[0].tbs)
    grids, ces, llrs = [], [], []
    for i, c in enumerate(cfgs):
        H = channel(c, 50 + i, taps=(1.0, 0.0, 0.0))
        g32, c32 = f32c(rx_grid(R.tx_grid(c, tb, qpp()), H, snr, 50 + i)), f32c(H)
        grids.append(g32)
        ces.append(c32)
        llrs.append(R.pdsch_llr(c, c128(g32).reshape(R.NSYMB, c.W),
                                c128(c32).reshape(c.nof_ports, R.NSYMB, c.W)).astype(np.float32))
    return cfgs, tb, grids, ces, llrs, need
