"""Two-antenna receive diversity (maximum-ratio combining) on top of tests/pdsch_ref.py: float64 numpy, extending its
conventions C5 / C6 to n_rx antennas.  grids[a] and ces[a] are antenna a's grid [14, W] and estimates [P, 14, W].

  TM1: x = sum_a y_a conj(h_a[0]) / (sum_a |h_a[0]|^2 + noise)
  TM2 (SFBC pair, notation of pdsch_ref.equalize): hh = sum_a (|h00_a|^2 + |h11_a|^2),
       x0 = sqrt2 sum_a (conj(h00_a) r0_a + h11_a conj(r1_a)) / hh,  x1 = sqrt2 sum_a (-h10_a conj(r0_a) + conj(h01_a) r1_a) / hh

With one antenna the expressions are evaluated in pdsch_ref.equalize's order, so the result is array_equal to it."""
import numpy as np

import pdsch_ref as R
import pdsch_ref_util as U


def equalize_rx(grids, ces, mask, tm, noise=0.01):
    """PDSCH symbols in mapping order, the antennas combined"""
    if tm != 2:
        num, den = 0, 0
        for g, ce in zip(grids, ces):
            y, h = g[mask], ce[0][mask]
            num = num + y * np.conj(h)
            den = den + np.abs(h) ** 2
        return num / (den + noise)
    hh, n0, n1 = 0, 0, 0
    for g, ce in zip(grids, ces):
        y, h0, h1 = g[mask], ce[0][mask], ce[1][mask]
        r0, r1 = y[0::2], y[1::2]
        h00, h01, h10, h11 = h0[0::2], h0[1::2], h1[0::2], h1[1::2]
        hh = hh + (np.abs(h00) ** 2 + np.abs(h11) ** 2)
        n0 = n0 + (np.conj(h00) * r0 + h11 * np.conj(r1))
        n1 = n1 + (-h10 * np.conj(r0) + np.conj(h01) * r1)
    x0 = np.sqrt(2) * n0 / hh
    x1 = np.sqrt(2) * n1 / hh
    return np.stack([x0, x1], 1).reshape(-1)


def pdsch_llr_rx(cfg, grids, ces, noise=0.01):
    x = equalize_rx(grids, ces, cfg.re_mask(), cfg.tm, noise)
    return R.descramble(R.demap(x, cfg.Qm), R.pdsch_c_init(cfg.rnti, cfg.sf, cfg.cell_id))


def half_band_channel(cfg, seed, a):
    """antenna a's test channel of the diversity scenario: U.channel(cfg, 100 seed + a) on one half of the band and
    nothing on the other (antenna 0 keeps k < W / 2, antenna 1 keeps k >= W / 2), so neither antenna alone carries
    the transport block"""
    H = U.channel(cfg, 100 * seed + a)
    k = np.arange(cfg.W)
    return H * ((k < cfg.W // 2) if a == 0 else (k >= cfg.W // 2))[None, None, :]


# ---- the diversity scenario (CPU test 4 pins it, GPU test (e) runs it on the device)
DIV_SEEDS = (0, 1, 2)
DIV_SNR_DB = 25.0
DIV_CASES = {"tm1_64qam": dict(nof_ports=1, Qm=6, tbs=2024), "tm2_16qam": dict(nof_ports=2, Qm=4, tbs=1000)}


def div_cfg(name, seed):
    return R.Cfg(cell_id=7 + seed, nof_prb=6, sf=1, cfi=1, **DIV_CASES[name])


def div_samples(name, seed):
    """(cfg, tb, [complex128 samples of antenna 0, of antenna 1]): one transmit grid through each antenna's half-band
    channel, each antenna with its own noise"""
    cfg = div_cfg(name, seed)
    tb = U.tb_bytes(900 + seed, cfg.tbs)
    grids = R.tx_grid(cfg, tb, U.qpp())
    iqs = [R.ofdm_tx(grids, half_band_channel(cfg, seed, a), DIV_SNR_DB, np.random.default_rng(0xD1700 + 10 * seed + a))
           for a in range(2)]
    return cfg, tb, iqs


# ---- two-antenna inputs of the demap stage (CPU test 3 and GPU test (b) share them)
_DEMAP_RX = {}


def demap_rx_inputs(cfgs):
    """per configuration: float32 interleaved grids [2][14 W] and estimates [2][P 14 W] of two antennas seeing the same
    PDSCH symbols through independent channels at 25 dB, with exactly known estimates (antenna 0 is the single-antenna
    case of test_gpu_pdsch_ref.test_demap_reference_grid_and_ce).  The TM2 equaliser divides by the sum over the
    antennas of |h00|^2 + |h11|^2: it is kept at >= 0.1 of its mean, for antenna 0 alone and for both."""
    key = tuple(id(c) for c in cfgs)
    if key not in _DEMAP_RX:
        out = []
        for i, c in enumerate(cfgs):
            Hs = [U.channel(c, 20 + i + 500 * a) for a in range(2)]
            if c.tm == 2:
                m = c.re_mask()
                hh = [np.abs(H[0][m][0::2]) ** 2 + np.abs(H[1][m][1::2]) ** 2 for H in Hs]
                for d in (hh[0], hh[0] + hh[1]):
                    assert d.min() >= 0.1 * d.mean(), (i, d.min() / d.mean())
            X = U.pdsch_symbol_grid(c, i)
            out.append(([U.f32c(U.rx_grid(X, H, 25.0, i + 500 * a)) for a, H in enumerate(Hs)], [U.f32c(H) for H in Hs]))
        _DEMAP_RX[key] = (cfgs, out)      # cfgs kept alive: the key is their identity
    return _DEMAP_RX[key][1]


def as_grids(cfg, g32s):
    return [U.c128(g).reshape(R.NSYMB, cfg.W) for g in g32s]


def as_ces(cfg, c32s):
    return [U.c128(c).reshape(cfg.nof_ports, R.NSYMB, cfg.W) for c in c32s]
