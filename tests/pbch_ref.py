"""Test helper (not product code): an independent PBCH transmitter and receiver (36.211 6.6, 36.212 5.3.1) in
numpy over oracle primitives -- or_crc16, or_conv_encode_tb, or_conv_rm_tx, or_conv_rm_rx, or_viterbi_tb,
or_gold, or_dft, or_cp_len, or_ofdm_rx, or_chest.

The receiver restates the equaliser and demapper formulas of the PDCCH path (eq_tm1, eq_tm2, qpsk_llr) in
float32, and its decode walks the same (candidate, ports P, depth f, phase phi) jobs in the same order as the
product: f ascending, then P = 1, 2, then phi ascending; first CRC match wins."""
import ctypes as C

import numpy as np

import oracle_lib as O

A, D, E, NRE, NB = 24, 40, 1920, 240, 480
CRC_MASK = {1: 0x0000, 2: 0xFFFF}     # 36.212 Table 5.3.1.1-1


def _lib():
    L = O.lib()
    f64 = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    L.or_dft.restype, L.or_dft.argtypes = None, [f64, f64, C.c_int, C.c_int]
    L.or_cp_len.restype, L.or_cp_len.argtypes = C.c_int, [C.c_uint32, C.c_uint32]
    return L


def re_list(cell_id, nof_prb):
    """240 REs, symbol then subcarrier: the 72 centre subcarriers of symbols 7..10 without the REs reserved for
    CRS of ports 0-3 in symbols 7 and 8 (k mod 3 = N_ID mod 3)"""
    W, k0 = 12 * nof_prb, 6 * nof_prb - 36
    out = []
    for l in range(7, 11):
        ks = np.arange(k0, k0 + 72)
        if l <= 8:
            ks = ks[ks % 3 != cell_id % 3]
        out.append(l * W + ks)
    return np.concatenate(out).astype(np.uint32)


def encode(bits24, ports):
    """the BCH TTI's 1920 rate-matched bits (not scrambled)"""
    L = _lib()
    a = np.ascontiguousarray(bits24, np.uint8)
    crc = L.or_crc16(a, A) ^ CRC_MASK[ports]
    c = np.concatenate([a, np.array([(crc >> (15 - i)) & 1 for i in range(16)], np.uint8)])
    d = np.zeros(3 * D, np.uint8)
    L.or_conv_encode_tb(c, D, d)
    e = np.zeros(E, np.uint8)
    L.or_conv_rm_tx(d, D, E, e)
    return e


def scr_bits(cell_id):
    c = np.zeros(E, np.uint8)
    _lib().or_gold(cell_id, c, E)
    return c


def symbols(cell_id, bits24, ports, phase):
    """the 240 QPSK symbols of the frame at 40 ms phase `phase`"""
    b = (encode(bits24, ports) ^ scr_bits(cell_id))[NB * phase:NB * (phase + 1)].astype(np.float64)
    return ((1 - 2 * b[0::2]) + 1j * (1 - 2 * b[1::2])) / np.sqrt(2.0)


def layer_grids(cell_id, nof_prb, bits24, ports, phase):
    """per-port grids [ports][14 * W] holding only the PBCH"""
    W = 12 * nof_prb
    x = symbols(cell_id, bits24, ports, phase)
    re = re_list(cell_id, nof_prb)
    g = np.zeros((ports, 14 * W), np.complex128)
    if ports == 1:
        g[0, re] = x
    else:   # 36.211 6.3.4.3: port 0 carries x0, x1; port 1 carries -conj(x1), conj(x0); all / sqrt 2
        x0, x1 = x[0::2], x[1::2]
        g[0, re[0::2]], g[0, re[1::2]] = x0 / np.sqrt(2), x1 / np.sqrt(2)
        g[1, re[0::2]], g[1, re[1::2]] = -np.conj(x1) / np.sqrt(2), np.conj(x0) / np.sqrt(2)
    return g


def tx(cell_id, nof_prb, ports, bits24, phase, h=None):
    """IQ (float32 interleaved, one subframe) of the PBCH alone: IDFT scaled 1 / sqrt N, CP, flat channel per port"""
    L = _lib()
    N = L.or_symbol_sz(nof_prb)
    W = 12 * nof_prb
    h = list(h) if h is not None else [1.0 + 0j, 0j]
    g = layer_grids(cell_id, nof_prb, bits24, ports, phase)
    z = np.zeros(15 * N, np.complex128)
    k = np.arange(W)
    bins = np.where(k < W // 2, N - W // 2 + k, k - W // 2 + 1)
    pos = 0
    for l in range(14):
        cp = L.or_cp_len(N, l % 7)
        if 7 <= l <= 10:
            for p in range(ports):
                X = np.zeros(2 * N)
                X[2 * bins], X[2 * bins + 1] = g[p, l * W:(l + 1) * W].real, g[p, l * W:(l + 1) * W].imag
                y = np.zeros(2 * N)
                L.or_dft(X, y, N, 1)
                t = (y[0::2] + 1j * y[1::2]) / np.sqrt(N)
                z[pos:pos + cp + N] += h[p] * np.concatenate([t[N - cp:], t])
        pos += cp + N
    out = np.zeros(2 * len(z), np.float32)
    out[0::2], out[1::2] = z.real, z.imag
    return out


def front(cell_id, nof_prb, ports, iq):
    """oracle OFDM RX + channel estimation of a subframe 0: (grid [14 W], ce [ports][14 W]) complex64"""
    L = _lib()
    cell = O.Cell(cell_id, nof_prb, ports)
    W = 12 * nof_prb
    grid = np.zeros(2 * 14 * W, np.float32)
    ce = np.zeros(2 * 14 * W * ports, np.float32)
    met = np.zeros(5, np.float32)
    L.or_ofdm_rx(C.byref(cell), np.ascontiguousarray(iq, np.float32), grid)
    L.or_chest(C.byref(cell), 0, grid, ce, met)
    return grid.view(np.complex64), ce.view(np.complex64).reshape(ports, 14 * W)


def _qpsk_llr(x):
    a = np.float32(0.70710678118)
    two = np.float32(2.0)
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    out = np.zeros(2 * len(x), np.float32)
    out[0::2] = ((xr - a) * (xr - a) - (xr + a) * (xr + a)) * two
    out[1::2] = ((xi - a) * (xi - a) - (xi + a) * (xi + a)) * two
    return out


def soft_bits(cell_id, nof_prb, ports, grid, ce, noise=0.0):
    """[2][480] float32, not descrambled: hypothesis 0 = one port (eq_tm1 on ce[0]), hypothesis 1 = two ports
    (eq_tm2 on consecutive RE pairs; zeros when the front end estimated one port)"""
    re = re_list(cell_id, nof_prb)
    out = np.zeros((2, NB), np.float32)
    y, h0 = grid[re], ce[0][re]
    f = np.float32
    yr, yi, hr, hi = y.real.astype(f), y.imag.astype(f), h0.real.astype(f), h0.imag.astype(f)
    den = hr * hr + hi * hi + f(noise)
    out[0] = _qpsk_llr(((yr * hr + yi * hi) / den) + 1j * ((yi * hr - yr * hi) / den))
    if ports == 2:
        h1 = ce[1][re]
        r0, r1 = y[0::2], y[1::2]
        h00, h01, h10, h11 = h0[0::2], h0[1::2], h1[0::2], h1[1::2]
        R = lambda v: v.real.astype(f)
        I = lambda v: v.imag.astype(f)
        hh = R(h00) * R(h00) + I(h00) * I(h00) + R(h11) * R(h11) + I(h11) * I(h11)
        hh = np.where(hh <= 0, f(1e-9), hh)
        s = f(1.41421356237) / hh
        x0r = s * ((R(h00) * R(r0) + I(h00) * I(r0)) + (R(h11) * R(r1) + I(h11) * I(r1)))
        x0i = s * ((R(h00) * I(r0) - I(h00) * R(r0)) + (I(h11) * R(r1) - R(h11) * I(r1)))
        x1r = s * (-(R(h10) * R(r0) + I(h10) * I(r0)) + (R(h01) * R(r1) + I(h01) * I(r1)))
        x1i = s * (-(I(h10) * R(r0) - R(h10) * I(r0)) + (R(h01) * I(r1) - I(h01) * R(r1)))
        x = np.zeros(NRE, np.complex64)
        x[0::2], x[1::2] = x0r + 1j * x0i, x1r + 1j * x1i
        out[1] = _qpsk_llr(x)
    return out


def jobs(n_frames, ports=(1, 2)):
    """(P, f, phi) in search order"""
    return [(P, f, phi) for f in range(1, n_frames + 1) for P in ports for phi in range(f - 1, 4)]


def decode_job(cell_id, frames, P, f, phi, scr=None):
    """frames: soft bits [n][2][480] of the candidate, oldest first.  Returns (crc match, bits[24])."""
    L = _lib()
    cs = scr if scr is not None else scr_bits(cell_id)
    e = np.zeros(E, np.float32)
    n = len(frames)
    for i in range(f):
        ph = phi - f + 1 + i
        v = np.asarray(frames[n - f + i][P - 1], np.float32)
        e[NB * ph:NB * (ph + 1)] = np.where(cs[NB * ph:NB * (ph + 1)] == 1, -v, v)
    d = np.zeros(3 * D, np.float32)
    L.or_conv_rm_rx(e, E, D, d)
    c = np.zeros(D, np.uint8)
    L.or_viterbi_tb(d, D, c)
    rx = 0
    for b in c[A:]:
        rx = (rx << 1) | int(b)
    return (L.or_crc16(c[:A].copy(), A) ^ rx) == CRC_MASK[P], c[:A].copy()


def decode(cell_id, frames, ports=(1, 2)):
    """first job that passes: (nof_ports, sfn_offset, n_frames_used, bits[24]) or None"""
    cs = scr_bits(cell_id)
    for P, f, phi in jobs(len(frames), ports):
        ok, bits = decode_job(cell_id, frames, P, f, phi, cs)
        if ok:
            return P, phi, f, bits
    return None


def mib_bits(nof_prb, phich_length, phich_resources, sfn):
    """the 24 MIB bits (36.331): 3 bandwidth bits, phich-Duration, 2 phich-Resource bits, 8 SFN MSBs, 10 spare"""
    bw = (6, 15, 25, 50, 75, 100).index(nof_prb)
    s = f"{bw:03b}{phich_length:01b}{phich_resources:02b}{(sfn >> 2) & 0xFF:08b}" + "0" * 10
    return np.array([int(ch) for ch in s], np.uint8)


def awgn(iq, snr_db, seed):
    """complex AWGN of variance 10^(-snr/10) per sample (= per RE: the OFDM scaling is unitary)"""
    if snr_db is None:
        return iq
    rng = np.random.default_rng(seed)
    return (iq + rng.normal(0.0, np.sqrt(10 ** (-snr_db / 10) / 2), len(iq))).astype(np.float32)
