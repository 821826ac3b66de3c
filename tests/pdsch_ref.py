"""Independent float64 reference of the LTE PDSCH downlink chain (numpy only).

A second restatement of what oracle/*.c and the HIP kernels compute, written from 3GPP TS 36.211 /
36.212 in a shape that shares no index arithmetic with either: the sub-block interleaver is an
actual R x 32 matrix, the PDSCH resource elements are a boolean [14, 12 N_RB] mask with regions
knocked out, the demapper searches the complex constellation, the DFT is numpy's.  It imports
nothing but numpy; tables that are pure transcription (QPP f1 / f2, TBS) are passed in by the caller.
Everything is float64 / complex128.

Spec-defined parts (36.212 5.1.1-5.1.4, 5.3.2; 36.211 6.3, 6.7, 6.10.1, 6.12, 7.1, 7.2) have one right
answer.  The receive side additionally follows CONVENTIONS of this project's reading of srsLTE (tagged
[X] in SURVEY.md, listed at the top of oracle/o_rx.c); they are named as conventions where they are
implemented and this module pins their arithmetic, not their choice:
  C1  rate matching uses N_cb = K_w (no soft-buffer limitation, 36.212 5.1.4.1.2 with N_IR large)
  C2  PSS / SSS / PBCH symbols exclude the whole central 72 subcarriers from the PDSCH
  C3  OFDM receive: unnormalised forward DFT of the samples after the CP (transmit: 1 / sqrt(N))
  C4  channel estimation: LS, 3-tap smoothing [0.1 0.8 0.1] with renormalised edges, linear interpolation
      with edge extrapolation in frequency, then in time over the pilot symbols {0, 4, 7, 11}
      (symbols <= 4 from (0, 4), 5..7 from (4, 7), >= 8 from (7, 11)); metrics rsrp = mean |p|^2 of port 0,
      rssi = mean over the pilot symbols of sum_k |y|^2, rsrq = N_RB rsrp / rssi,
      noise = mean |p - p_smooth|^2 over all ports, snr = rsrp / noise
  C5  TM1 equaliser x = y conj(h) / (|h|^2 + sigma^2), sigma^2 = 0.01 passed in
  C6  TM2 equaliser with hh = |h00|^2 + |h11|^2 (port 0 at the pair's first RE, port 1 at its second)
  C7  max-log demapper, LLR = (min_{b=0} d^2 - min_{b=1} d^2) / sigma^2 with sigma^2 = 0.5; LLR > 0 means bit 1
  C8  filler bits enter the decoder as a large negative LLR (known zero); payload bytes MSB first
"""
import numpy as np

NULL = -1            # <NULL> of 36.212 5.1.3 / 5.1.4 in integer streams
NSYMB = 14           # normal CP
FILLER_LLR = -1e4    # C8

# 36.212 Table 5.1.3-3, the K column: its regular structure, not the table
CB_SIZES = np.concatenate([np.arange(40, 512, 8), np.arange(512, 1024, 16), np.arange(1024, 2048, 32),
                           np.arange(2048, 6144 + 1, 64)])

CRC24A = (24, [24, 23, 18, 17, 14, 11, 10, 7, 6, 5, 4, 3, 1, 0])   # exponents of g_CRC24A(D), 36.212 5.1.1
CRC24B = (24, [24, 23, 6, 5, 1, 0])
CRC16 = (16, [16, 12, 5, 0])


# ------------------------------------------------------------------------------------------ bit level
def crc(bits, gen):
    """Parity bits p_0 .. p_{L-1} of 36.212 5.1.1: remainder of a(D) D^L by g(D) over GF(2), by long division."""
    return crc_many(np.asarray(bits)[None, :], gen)[0]


def crc_many(bits, gen):
    """crc of n sequences of one length: bits[n, A] -> parity[n, L]"""
    L, exps = gen
    g = np.zeros(L + 1, np.uint8)
    g[[L - e for e in exps]] = 1
    bits = np.asarray(bits, np.uint8) & 1
    n, A = bits.shape
    r = np.concatenate([bits, np.zeros((n, L), np.uint8)], 1)
    if n == 1:
        for i in range(A):
            if r[0, i]:          # one sequence: skip the zero steps
                r[0, i:i + L + 1] ^= g
    else:
        for i in range(A):
            r[:, i:i + L + 1] ^= g[None, :] * r[:, i:i + 1]
    return r[:, A:]


def gold(c_init, n):
    """36.211 7.2: c(i) = x1(i + Nc) + x2(i + Nc), Nc = 1600, 28 recurrence steps per numpy operation."""
    Nc, tot = 1600, 1600 + n + 31 + 28
    x1 = np.zeros(tot, np.uint8)
    x2 = np.zeros(tot, np.uint8)
    x1[0] = 1
    x2[:31] = [(c_init >> i) & 1 for i in range(31)]
    for a in range(0, tot - 31 - 28 + 1, 28):
        x1[a + 31:a + 59] = x1[a + 3:a + 31] ^ x1[a:a + 28]
        x2[a + 31:a + 59] = x2[a + 3:a + 31] ^ x2[a + 2:a + 30] ^ x2[a + 1:a + 29] ^ x2[a:a + 28]
    return (x1[Nc:Nc + n] ^ x2[Nc:Nc + n]).astype(np.uint8)


def segment(B):
    """36.212 5.1.2 for B bits (TB + CRC24A): dict C, Kp, Km, Cp, Cm, F."""
    Z = 6144
    if B <= Z:
        C, Bp = 1, B
    else:
        C = -(-B // (Z - 24))
        Bp = B + 24 * C
    Kp = int(CB_SIZES[CB_SIZES * C >= Bp][0])
    if C == 1:
        Cp, Km, Cm = 1, 0, 0
    else:
        Km = int(CB_SIZES[CB_SIZES < Kp][-1])
        Cm = (C * Kp - Bp) // (Kp - Km)
        Cp = C - Cm
    return dict(C=C, Kp=Kp, Km=Km, Cp=Cp, Cm=Cm, F=Cp * Kp + Cm * Km - Bp)


def _rsc(c):
    """One constituent encoder, 36.212 5.1.3.2.1: G(D) = [1, g1(D) / g0(D)], g0 = 1 + D^2 + D^3, g1 = 1 + D + D^3,
    as difference equations on the feedback sequence a_k; then the trellis termination of 5.1.3.2.2 (the switch in
    the lower position feeds the register back, so a_k = 0).  Returns (z[n, K], tail x[n, 3], tail z[n, 3]).
    c: [n, K] -- n blocks advance together, block i in bit i of a Python integer (GF(2) addition is ^)."""
    n, K = c.shape
    nb = (n + 7) // 8
    cols = np.packbits(c, axis=0, bitorder="little")                     # [nb, K]
    c = [int.from_bytes(cols[:, k].tobytes(), "little") for k in range(K)]
    a = [0] * (K + 6)                  # a[k + 3] = a_k, zero initial state
    out = [0] * (K + 6)                # z_0 .. z_{K-1}, then x_K z_K x_{K+1} z_{K+1} x_{K+2} z_{K+2}
    for k in range(K):
        ak = c[k] ^ a[k + 1] ^ a[k]                      # a_k = c_k + a_{k-2} + a_{k-3}
        a[k + 3] = ak
        out[k] = ak ^ a[k + 2] ^ a[k]                    # z_k = a_k + a_{k-1} + a_{k-3}
    for j in range(3):
        k = K + j
        out[K + 2 * j] = a[k + 1] ^ a[k]                 # x_k = a_{k-2} + a_{k-3}
        out[K + 2 * j + 1] = a[k + 2] ^ a[k]             # a_k = 0
    raw = np.frombuffer(b"".join(v.to_bytes(nb, "little") for v in out), np.uint8).reshape(K + 6, nb)
    bits = np.unpackbits(raw, axis=1, bitorder="little")[:, :n].T        # [n, K + 6]
    return bits[:, :K], bits[:, K::2], bits[:, K + 1::2]


def qpp_perm(K, f1, f2):
    i = np.arange(K, dtype=np.int64)
    return (f1 * i + f2 * i * i) % K


def turbo_encode(bits, f1, f2, F=0):
    """36.212 5.1.3.2: d[3, K + 4] (rows d0 / d1 / d2); F filler bits at the head are encoded as 0 and come out
    as NULL in d0 and d1."""
    return turbo_encode_many(np.asarray(bits)[None, :], f1, f2, F)[0]


def turbo_encode_many(bits, f1, f2, F=0):
    """turbo_encode of n blocks of one size: bits[n, K] -> d[n, 3, K + 4]"""
    c = np.array(bits, np.uint8) & 1
    n, K = c.shape
    c[:, :F] = 0
    z, xt, zt = _rsc(c)
    zp, xpt, zpt = _rsc(c[:, qpp_perm(K, f1, f2)])
    d = np.zeros((n, 3, K + 4), np.int64)
    d[:, 0, :K], d[:, 1, :K], d[:, 2, :K] = c, z, zp
    d[:, 0, K:] = np.stack([xt[:, 0], zt[:, 1], xpt[:, 0], zpt[:, 1]], 1)      # 36.212 5.1.3.2.2
    d[:, 1, K:] = np.stack([zt[:, 0], xt[:, 2], zpt[:, 0], xpt[:, 2]], 1)
    d[:, 2, K:] = np.stack([xt[:, 1], zt[:, 2], xpt[:, 1], zpt[:, 2]], 1)
    d[:, :2, :F] = NULL
    return d


P_COLS = np.array([int(format(i, "05b")[::-1], 2) for i in range(32)])   # Table 5.1.4-1 is the 5-bit reversal


def _subblock(y, shift):
    """36.212 5.1.4.1.1: N_D NULLs in front, written row by row into an R x 32 matrix, columns permuted, read column by
    column.  shift = 1 is the third stream's pi(k) = (P(k / R) + 32 (k mod R) + 1) mod K_pi: the same read-out of
    the sequence advanced by one position (cyclically)."""
    D = len(y)
    R = -(-D // 32)
    full = np.concatenate([np.full(32 * R - D, NULL, np.int64), y])
    mat = np.roll(full, -shift).reshape(R, 32)
    return mat[:, P_COLS].T.reshape(-1)


def circular_buffer(d):
    """w of 36.212 5.1.4.1.2 from d[3, D]: v0, then v1 and v2 interlaced."""
    v = [_subblock(d[i], int(i == 2)) for i in range(3)]
    return np.concatenate([v[0], np.stack([v[1], v[2]], 1).reshape(-1)])


def rm_k0(K, rv):
    R = -(-(K + 4) // 32)
    Ncb = 3 * 32 * R          # C1
    return R * (2 * (-(-Ncb // (8 * R))) * rv + 2)


def rate_match(d, K, F, E, rv):
    """36.212 5.1.4.1.2 bit selection with N_cb = K_w (C1): E values of d[3, K + 4] (any integers >= 0; d0 / d1 of
    the F filler positions are made NULL)."""
    d = np.array(d, np.int64)
    assert d.shape == (3, K + 4)
    d[:2, :F] = NULL
    w = circular_buffer(d)
    seq = np.roll(w, -rm_k0(K, rv))
    return np.resize(seq[seq != NULL], E)


def rm_index_map(K, F, E, rv):
    """position in d.reshape(-1) (row-major [3, K + 4]) that each of the E transmitted bits carries"""
    return rate_match(np.arange(3 * (K + 4)).reshape(3, K + 4), K, F, E, rv)


def rm_E(G, C, Qm, NL, r):
    """36.212 5.1.4.1.2: E of code block r."""
    Gp = G // (NL * Qm)
    gamma = Gp % C
    return NL * Qm * (Gp // C) if r <= C - gamma - 1 else NL * Qm * (-(-Gp // C))


def bytes_to_bits(tb):
    return np.unpackbits(np.asarray(tb, np.uint8))          # MSB first (C8)


def dlsch_code_blocks(tbs, tb_bits):
    """36.212 5.3.2.1-5.3.2.2: CRC24A, segmentation, filler bits, CRC24B -> (segment dict, list of (K, F, c bits))"""
    b = np.concatenate([tb_bits, crc(tb_bits, CRC24A)])
    sg = segment(tbs + 24)
    out, pos = [], 0
    for r in range(sg["C"]):
        K = sg["Km"] if r < sg["Cm"] else sg["Kp"]
        F = sg["F"] if r == 0 else 0
        L = 24 if sg["C"] > 1 else 0
        n = K - L - F
        c = np.concatenate([np.zeros(F, np.uint8), b[pos:pos + n]])
        pos += n
        if L:
            c = np.concatenate([c, crc(c, CRC24B)])
        out.append((K, F, c))
    assert pos == len(b)
    return sg, out


def dlsch_encode(tbs, tb_bits, G, Qm, NL, rv, qpp):
    """transport block -> the G coded bits f (36.212 5.3.2); qpp: K -> (f1, f2)"""
    sg, cbs = dlsch_code_blocks(tbs, tb_bits)
    f = []
    for r, (K, F, c) in enumerate(cbs):
        d = turbo_encode(c, *qpp[K], F)
        f.append(rate_match(d, K, F, rm_E(G, sg["C"], Qm, NL, r), rv))
    return np.concatenate(f).astype(np.uint8)


# ------------------------------------------------------------------------------------------ symbols and grid
def pdsch_c_init(rnti, sf, cell_id, q=0):
    return rnti * 2 ** 14 + q * 2 ** 13 + sf * 2 ** 9 + cell_id      # 36.211 6.3.1, floor(ns / 2) = sf


def scramble(bits, c_init):
    return np.asarray(bits, np.uint8) ^ gold(c_init, len(bits))


def modulate(bits, Qm):
    """36.211 7.1.2-7.1.4 in their closed form: bits b(i), b(i+1), ... -> I from the even, Q from the odd ones."""
    b = 1.0 - 2.0 * np.asarray(bits, np.float64).reshape(-1, Qm)
    if Qm == 2:
        return (b[:, 0] + 1j * b[:, 1]) / np.sqrt(2)
    if Qm == 4:
        return (b[:, 0] * (2 - b[:, 2]) + 1j * b[:, 1] * (2 - b[:, 3])) / np.sqrt(10)
    if Qm == 6:
        return (b[:, 0] * (4 - b[:, 2] * (2 - b[:, 4])) + 1j * b[:, 1] * (4 - b[:, 3] * (2 - b[:, 5]))) / np.sqrt(42)
    raise ValueError(Qm)


SFBC_W = np.array([[1, 0, 1j, 0], [0, -1, 0, 1j], [0, 1, 0, 1j], [1, 0, -1j, 0]]) / np.sqrt(2)   # 36.211 6.3.4.3


def sfbc(x):
    """Transmit diversity on two ports, 36.211 6.3.3.3 + 6.3.4.3: x[2n] -> y[2, 2n] through the spec's matrix."""
    x = np.asarray(x, np.complex128).reshape(-1, 2)
    v = np.stack([x[:, 0].real, x[:, 1].real, x[:, 0].imag, x[:, 1].imag])      # [4, n]
    y = SFBC_W @ v                                                             # y0(2i) y1(2i) y0(2i+1) y1(2i+1)
    return np.stack([np.stack([y[0], y[2]], 1).reshape(-1), np.stack([y[1], y[3]], 1).reshape(-1)])


def crs(cell_id, ns, l, port, nof_prb):
    """36.211 6.10.1: (values r_{l,ns}(m'), subcarriers k) of the CRS of `port` in symbol l (0 or 4) of slot ns."""
    c_init = 2 ** 10 * (7 * (ns + 1) + l + 1) * (2 * cell_id + 1) + 2 * cell_id + 1        # N_CP = 1
    c = gold(c_init, 4 * 110).astype(np.float64)
    r = ((1 - 2 * c[0::2]) + 1j * (1 - 2 * c[1::2])) / np.sqrt(2)
    m = np.arange(2 * nof_prb)
    v = {(0, 0): 0, (0, 4): 3, (1, 0): 3, (1, 4): 0}[(port, l)]
    return r[m + 110 - nof_prb], 6 * m + (v + cell_id % 6) % 6


def ctrl_symbols(nof_prb, cfi):
    return cfi + 1 if nof_prb <= 10 else cfi      # 36.212 5.3.4 / 36.211 Table 6.7-1


def pdsch_re_mask(cell_id, nof_prb, nof_ports, cfi, sf, prb_slots):
    """Boolean [14, 12 N_RB] of the PDSCH's resource elements (36.211 6.3.5); prb_slots[2, N_RB]: PRB used in
    slot 0 / 1.  Row-major order of the True entries is the mapping order (k first, then l)."""
    W = 12 * nof_prb
    m = np.repeat(np.repeat(np.asarray(prb_slots, bool), 12, axis=1), 7, axis=0)    # [14, W]
    m[:ctrl_symbols(nof_prb, cfi)] = False
    for l in (0, 4, 7, 11):
        for p in range(nof_ports):
            m[l, crs(cell_id, 0, l % 7, p, nof_prb)[1]] = False
    mid = slice(W // 2 - 36, W // 2 + 36)                                           # C2
    if sf in (0, 5):
        m[5:7, mid] = False          # SSS, PSS: the last two symbols of slot 0
    if sf == 0:
        m[7:11, mid] = False         # PBCH: the first four symbols of slot 1
    return m


CFI_WORDS = {1: [0, 1, 1], 2: [1, 0, 1], 3: [1, 1, 0]}      # 36.212 Table 5.3.4-1: the period of each code word


def pcfich(cell_id, nof_prb, nof_ports, cfi, sf):
    """36.211 6.7: (symbols per port [P, 16], subcarriers of symbol 0 [16])"""
    b = np.resize(CFI_WORDS[cfi], 32).astype(np.uint8)
    b = scramble(b, (sf + 1) * (2 * cell_id + 1) * 2 ** 9 + cell_id)
    d = modulate(b, 2)
    y = d[None, :] if nof_ports == 1 else sfbc(d)
    W = 12 * nof_prb
    kbar = 6 * (cell_id % (2 * nof_prb))
    ks = []
    for i in range(4):
        k0 = (kbar + (i * nof_prb // 2) * 6) % W
        reg = np.arange(k0, k0 + 6)
        ks.append(reg[reg % 3 != cell_id % 3])     # REG of symbol 0: CRS of ports 0 and 1 assumed (6.2.4)
    return y, np.concatenate(ks)


class Cfg:
    """One PDSCH subframe.  prb_slots[2, N_RB] bool (default: every PRB in both slots)."""

    def __init__(self, cell_id=1, nof_prb=6, nof_ports=1, sf=1, cfi=1, tm=None, rnti=0x46, rv=0, tbs=16, Qm=2,
                 prb_slots=None, NL=None):
        self.cell_id, self.nof_prb, self.nof_ports, self.sf, self.cfi = cell_id, nof_prb, nof_ports, sf, cfi
        self.tm = tm if tm is not None else (2 if nof_ports == 2 else 1)
        self.rnti, self.rv, self.tbs, self.Qm = rnti, rv, tbs, Qm
        self.prb_slots = np.ones((2, nof_prb), bool) if prb_slots is None else np.asarray(prb_slots, bool)
        self.NL = NL if NL is not None else (2 if self.tm == 2 else 1)

    @property
    def W(self):
        return 12 * self.nof_prb

    def re_mask(self):
        return pdsch_re_mask(self.cell_id, self.nof_prb, self.nof_ports, self.cfi, self.sf, self.prb_slots)

    @property
    def G(self):
        return int(self.re_mask().sum()) * self.Qm


def tx_grid(cfg, tb, qpp):
    """Per-port resource grids [P, 14, 12 N_RB] of one subframe: PDSCH of transport block tb (bytes), CRS, PCFICH."""
    mask = cfg.re_mask()
    G = int(mask.sum()) * cfg.Qm
    f = dlsch_encode(cfg.tbs, bytes_to_bits(tb)[:cfg.tbs], G, cfg.Qm, cfg.NL, cfg.rv, qpp)
    x = modulate(scramble(f, pdsch_c_init(cfg.rnti, cfg.sf, cfg.cell_id)), cfg.Qm)
    grids = np.zeros((cfg.nof_ports, NSYMB, cfg.W), np.complex128)
    if cfg.tm == 2:
        y = sfbc(x)
        for p in range(2):
            grids[p][mask] = y[p]
    else:
        grids[0][mask] = x
    for p in range(cfg.nof_ports):
        for l in (0, 4, 7, 11):
            r, k = crs(cfg.cell_id, 2 * cfg.sf + l // 7, l % 7, p, cfg.nof_prb)
            grids[p, l, k] = r
    y, k = pcfich(cfg.cell_id, cfg.nof_prb, cfg.nof_ports, cfg.cfi, cfg.sf)
    grids[:, 0, k] = y
    return grids


# ------------------------------------------------------------------------------------------ OFDM
def symbol_sz(nof_prb):
    return {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}[nof_prb]


def cp_lens(N):
    """36.211 6.12, normal CP: 160 samples for l = 0 of each slot and 144 otherwise at N = 2048"""
    return [(160 if l % 7 == 0 else 144) * N // 2048 for l in range(NSYMB)]


def bins(nof_prb):
    """DFT bin of subcarrier k: k - 6 N_RB for the lower half, k - 6 N_RB + 1 for the upper (DC unused)"""
    W, N = 12 * nof_prb, symbol_sz(nof_prb)
    k = np.arange(W)
    return np.where(k < W // 2, k - W // 2, k - W // 2 + 1) % N


def ofdm_tx(grids, H=None, snr_db=None, rng=None):
    """Per-port grids -> complex128 samples of one subframe.  H[port, l, k]: frequency response applied per RE before
    the IFFT (any function of symbol and subcarrier; None = 1).  IFFT with 1 / sqrt(N) scaling (C3), cyclic prefix.
    snr_db: AWGN of variance 10^(-snr / 10) per complex sample from rng."""
    P, _, W = grids.shape
    nof_prb = W // 12
    N = symbol_sz(nof_prb)
    Y = grids if H is None else grids * H
    X = np.zeros((NSYMB, N), np.complex128)
    X[:, bins(nof_prb)] = Y.sum(0)
    x = np.fft.ifft(X, axis=1) * np.sqrt(N)
    out = np.concatenate([np.concatenate([x[l, N - cp:], x[l]]) for l, cp in enumerate(cp_lens(N))])
    if snr_db is not None:
        s = np.sqrt(10.0 ** (-snr_db / 10.0) / 2.0)
        out = out + s * (rng.standard_normal(len(out)) + 1j * rng.standard_normal(len(out)))
    return out


def ofdm_rx(iq, nof_prb):
    """samples -> grid [14, 12 N_RB] (C3)"""
    N = symbol_sz(nof_prb)
    iq = np.asarray(iq, np.complex128)
    pos, rows = 0, []
    for cp in cp_lens(N):
        rows.append(np.fft.fft(iq[pos + cp:pos + cp + N])[bins(nof_prb)])
        pos += cp + N
    return np.array(rows)


# ------------------------------------------------------------------------------------------ receiver
PILOT_L = np.array([0, 4, 7, 11])


def _lin(x, xp, fp):
    """linear interpolation through the points (xp, fp), extended beyond both ends with the end segments' slopes"""
    i = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, len(xp) - 2)
    t = (x - xp[i]) / (xp[i + 1] - xp[i])
    return fp[..., i] + t * (fp[..., i + 1] - fp[..., i])


def chest(grid, cell_id, nof_prb, nof_ports, sf):
    """Channel estimates ce[P, 14, 12 N_RB] and metrics [rsrp, rssi, rsrq, noise, snr] (C4)."""
    W = 12 * nof_prb
    ce = np.zeros((nof_ports, NSYMB, W), np.complex128)
    kern = np.array([0.1, 0.8, 0.1])
    noise, rsrp = [], None
    for p in range(nof_ports):
        rows = []
        for l in PILOT_L:
            r, k = crs(cell_id, 2 * sf + l // 7, l % 7, p, nof_prb)
            ls = grid[l, k] * np.conj(r)
            sm = np.convolve(ls, kern, mode="same")
            sm[0] = (0.8 * ls[0] + 0.1 * ls[1]) / 0.9
            sm[-1] = (0.1 * ls[-2] + 0.8 * ls[-1]) / 0.9
            noise.append(np.abs(ls - sm) ** 2)
            if p == 0:
                rsrp = np.abs(ls) ** 2 if rsrp is None else np.concatenate([rsrp, np.abs(ls) ** 2])
            rows.append(_lin(np.arange(W, dtype=np.float64), k.astype(np.float64), sm))
        rows = np.array(rows)                                   # [4, W]
        # time: _lin's end-segment rule is the convention's: symbols 0..4 from (0, 4), 5..7 from (4, 7), 8..13 from (7, 11)
        ce[p] = _lin(np.arange(NSYMB, dtype=np.float64), PILOT_L.astype(np.float64), rows.T).T
    rsrp = rsrp.mean()
    rssi = (np.abs(grid[PILOT_L]) ** 2).sum(1).mean()
    noise = np.concatenate(noise).mean()
    return ce, np.array([rsrp, rssi, nof_prb * rsrp / rssi, noise, rsrp / noise if noise > 0 else 0.0])


def equalize(grid, ce, mask, tm, noise=0.01):
    """PDSCH symbols in mapping order: TM1 C5, TM2 C6"""
    y = grid[mask]
    if tm != 2:
        h = ce[0][mask]
        return y * np.conj(h) / (np.abs(h) ** 2 + noise)
    h0, h1 = ce[0][mask], ce[1][mask]
    r0, r1 = y[0::2], y[1::2]
    h00, h01, h10, h11 = h0[0::2], h0[1::2], h1[0::2], h1[1::2]
    hh = np.abs(h00) ** 2 + np.abs(h11) ** 2
    x0 = np.sqrt(2) * (np.conj(h00) * r0 + h11 * np.conj(r1)) / hh
    x1 = np.sqrt(2) * (-h10 * np.conj(r0) + np.conj(h01) * r1) / hh
    return np.stack([x0, x1], 1).reshape(-1)


def demap(x, Qm, sigma2=0.5):
    """max-log LLRs by a search over the 2^Qm complex constellation points (C7)"""
    M = 1 << Qm
    labels = (np.arange(M)[:, None] >> np.arange(Qm - 1, -1, -1)) & 1          # [M, Qm], b(i) first
    pts = modulate(labels.reshape(-1), Qm)
    out = np.zeros((len(x), Qm))
    for a in range(0, len(x), 4096):
        d2 = np.abs(x[a:a + 4096, None] - pts[None, :]) ** 2
        for j in range(Qm):
            out[a:a + 4096, j] = (d2[:, labels[:, j] == 0].min(1) - d2[:, labels[:, j] == 1].min(1)) / sigma2
    return out.reshape(-1)


def descramble(llr, c_init):
    return np.where(gold(c_init, len(llr)) == 1, -llr, llr)


def pdsch_llr(cfg, grid, ce, noise=0.01):
    x = equalize(grid, ce, cfg.re_mask(), cfg.tm, noise)
    return descramble(demap(x, cfg.Qm), pdsch_c_init(cfg.rnti, cfg.sf, cfg.cell_id))


def rx_front(cfg, iq):
    """(grid, ce, metrics, llr) of one subframe's samples"""
    grid = ofdm_rx(iq, cfg.nof_prb)
    ce, met = chest(grid, cfg.cell_id, cfg.nof_prb, cfg.nof_ports, cfg.sf)
    return grid, ce, met, pdsch_llr(cfg, grid, ce)


def rate_dematch(e, K, F, rv, soft=None):
    """HARQ combine of E soft bits into soft[3, K + 4] through the transmit index map (repeated positions add);
    returns (soft, decoder input with the filler positions of d0 / d1 at FILLER_LLR)"""
    soft = np.zeros(3 * (K + 4)) if soft is None else soft.reshape(-1).copy()
    np.add.at(soft, rm_index_map(K, F, len(e), rv), e)
    soft = soft.reshape(3, K + 4)
    d = soft.copy()
    d[:2, :F] = FILLER_LLR
    return soft, d


# trellis of the constituent code from its difference equations: state (a_{k-1}, a_{k-2}, a_{k-3})
_ST = [(s1, s2, s3) for s1 in (0, 1) for s2 in (0, 1) for s3 in (0, 1)]
_NEXT = np.zeros((8, 2), int)
_PAR = np.zeros((8, 2), int)
for _i, (_s1, _s2, _s3) in enumerate(_ST):
    for _u in (0, 1):
        _a = _u ^ _s2 ^ _s3
        _NEXT[_i, _u] = _ST.index((_a, _s1, _s2))
        _PAR[_i, _u] = _a ^ _s1 ^ _s3
# the two (state, input) pairs entering each state, as flat indices 2 s + u
_PRED = np.array([[2 * s + u for s in range(8) for u in (0, 1) if _NEXT[s, u] == n] for n in range(8)])


def _max_log_map(Ls, Lp, La, K):
    """One constituent max-log-MAP over K information steps + 3 termination steps; LLR > 0 means bit 1 (C7).
    Ls / Lp have K + 3 entries (tail included), La K.  Returns the a-posteriori LLRs [K]."""
    n = K + 3
    sys = Ls.copy()
    sys[:K] += La
    gam = np.zeros((n, 8, 2))
    for u in (0, 1):
        gam[:, :, u] = u * sys[:, None] + _PAR[None, :, u] * Lp[:, None]
    NEG = -1e300
    al = np.full((n + 1, 8), NEG)
    al[0, 0] = 0.0
    for k in range(n):
        c = (al[k][:, None] + gam[k]).reshape(-1)
        nx = np.maximum(c[_PRED[:, 0]], c[_PRED[:, 1]])
        al[k + 1] = nx - nx.max()
    be = np.full((n + 1, 8), NEG)
    be[n, 0] = 0.0
    for k in range(n - 1, -1, -1):
        b = (be[k + 1][_NEXT] + gam[k]).max(1)
        be[k] = b - b.max()
    t = al[:K, :, None] + gam[:K] + be[1:K + 1][:, _NEXT]
    return t[:, :, 1].max(1) - t[:, :, 0].max(1)


def turbo_decode(d, f1, f2, n_its=8, stop=None):
    """Textbook max-log-MAP turbo decoder in float64.  d[3, K + 4] soft bits (LLR > 0: bit 1) in the encoder's
    output layout; stop(bits) -> True ends the iterations early.  Returns (bits, iterations)."""
    K = d.shape[1] - 4
    pi = qpp_perm(K, f1, f2)
    t0, t1, t2 = d[0, K:], d[1, K:], d[2, K:]
    Ls1 = np.concatenate([d[0, :K], [t0[0], t2[0], t1[1]]])      # x_K x_{K+1} x_{K+2}
    Lp1 = np.concatenate([d[1, :K], [t1[0], t0[1], t2[1]]])      # z_K z_{K+1} z_{K+2}
    Ls2 = np.concatenate([d[0, :K][pi], [t0[2], t2[2], t1[3]]])
    Lp2 = np.concatenate([d[2, :K], [t1[2], t0[3], t2[3]]])
    La = np.zeros(K)
    bits = np.zeros(K, np.uint8)
    for it in range(1, n_its + 1):
        L1 = _max_log_map(Ls1, Lp1, La, K)
        e1 = L1 - Ls1[:K] - La
        L2 = _max_log_map(Ls2, Lp2, e1[pi], K)
        e2 = L2 - Ls2[:K] - e1[pi]
        La = np.zeros(K)
        La[pi] = e2
        full = np.zeros(K)
        full[pi] = L2
        bits = (full > 0).astype(np.uint8)
        if stop is not None and stop(bits):
            break
    return bits, it


def dlsch_decode(cfg, llr, qpp, soft=None, n_its=8):
    """Rate de-matching (+ HARQ combine into soft, a list of per-code-block arrays or None), turbo decoding with CRC
    early stop, TB assembly.  Returns (crc_ok, payload bytes, soft)."""
    sg = segment(cfg.tbs + 24)
    C = sg["C"]
    soft = [None] * C if soft is None else soft
    b, pos, new_soft = [], 0, []
    for r in range(C):
        K = sg["Km"] if r < sg["Cm"] else sg["Kp"]
        F = sg["F"] if r == 0 else 0
        E = rm_E(len(llr), C, cfg.Qm, cfg.NL, r)
        s, d = rate_dematch(llr[pos:pos + E], K, F, cfg.rv, soft[r])
        pos += E
        new_soft.append(s)
        gen = CRC24A if C == 1 else CRC24B
        bits, _ = turbo_decode(d, *qpp[K], n_its=n_its, stop=lambda x: np.array_equal(crc(x[:-24], gen), x[-24:]))
        b.append(bits[F:K - (24 if C > 1 else 0)])
    b = np.concatenate(b)
    ok = np.array_equal(crc(b[:-24], CRC24A), b[-24:])
    return ok, np.packbits(b[:cfg.tbs]), new_soft
