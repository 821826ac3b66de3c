"""Reference PUSCH transmitter with a variable symbol count (TEST INFRASTRUCTURE ONLY): 36.212 5.2.2.6-5.2.2.8 and
36.211 5.3 with N = 12 - n_srs data symbols and N_symb^PUSCH-initial = n_symb_initial in the Q' formulas.

The oracle (oracle/o_ul.c) knows only 12 symbols.  This composes its N-independent primitives (or_cbsegm, or_tcod,
or_rm_E, or_rm_tx, or_gold, or_ack_block / or_ri_block, or_cqi_rm32, or_crc*, or_dft_m, or_dmrs_pusch, or_scfdma_tx)
and restates in numpy what it does not expose: the Q' formulas, the CQI convolutional code with its 5.1.4.2 rate
matching, the multiplexer, the C_mux-column channel interleaver, scrambling with the UCI placeholders and the
modulation.  Every function takes the oracle's UlCfg (oracle_lib.ul_cfg) plus n_srs and n_symb_initial (0 = 12 -
n_srs).  At n_srs = 0 it must equal or_ulsch_encode bit for bit and or_pusch_encode in IQ (tests/test_pusch_ref.py).
"""
import ctypes as C

import numpy as np

import oracle_lib as O

# 36.213 Tables 8.6.3-1 (HARQ-ACK, I 0..14), 8.6.3-2 (RI, I 0..12), 8.6.3-3 (CQI, I 2..15): beta_offset x 8
BETA8_ACK = (16, 20, 25, 32, 40, 50, 64, 80, 101, 127, 160, 248, 400, 640, 1008)
BETA8_RI = (10, 13, 16, 20, 25, 32, 40, 50, 64, 80, 101, 127, 160)
BETA8_CQI = (0, 0, 9, 10, 11, 13, 14, 16, 18, 20, 23, 25, 28, 32, 40, 50)
RI_COLS, ACK_COLS = (1, 4, 7, 10), (2, 3, 8, 9)          # 36.212 Tables 5.2.2.8-1 / -2, normal CP
FFT_SIZE = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}


def n_symb(n_srs):
    return 12 - n_srs


def segm(tbs):
    s = O.CbSegm()
    assert O.lib().or_cbsegm(tbs, C.byref(s)) == 0
    return s


def cb_sizes(s):
    return [s.Km if r < s.Cm else s.Kp for r in range(s.C)]


def resource(c, n_srs=0, n_symb_initial=0):
    """dict(n_symb, G, q_ack, q_ri, q_cqi, C, E): 36.212 5.2.2.6 with N_symb^PUSCH-initial = n_symb_initial,
    M_sc^PUSCH-initial = M.  Q' = min(ceil(O M N_initial beta / sum K_r), cap): cap 4 M for HARQ-ACK and RI,
    N M - Q'_RI for CQI (O + 8 CRC bits above 11 bits)"""
    N, M = n_symb(n_srs), 12 * c.L_prb
    Ni = n_symb_initial or N
    s = segm(c.tbs)
    sumK = sum(cb_sizes(s))

    def qp(bits, beta8, cap):
        return min(-((-bits * M * Ni * beta8) // (8 * sumK)), cap)

    q_ack = qp(c.ack_len, BETA8_ACK[min(c.I_offset_ack, 14)], 4 * M) if c.ack_len else 0
    q_ri = qp(c.ri_len, BETA8_RI[c.I_offset_ri], 4 * M) if c.ri_len else 0
    q_cqi = qp(c.cqi_len + (8 if c.cqi_len > 11 else 0), BETA8_CQI[c.I_offset_cqi], N * M - q_ri) if c.cqi_len else 0
    G = (N * M - q_cqi - q_ri) * c.Qm
    E = [O.lib().or_rm_E(G, s.C, c.Qm, 1, r) for r in range(s.C)]
    return dict(n_symb=N, G=G, q_ack=q_ack, q_ri=q_ri, q_cqi=q_cqi, C=s.C, E=E)


# ---- CQI channel coding (36.212 5.2.2.6.4) ---------------------------------------------------------------
CONV_G = (0o133, 0o171, 0o165)                               # 5.1.3.1, constraint length 7
CONV_PERM = (1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31,
             0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30)   # Table 5.1.4-2


def conv_encode_tb(a):
    """tail-biting rate-1/3 code: d_k^(i) = sum_j g_i[j] c_(k-j mod D), g_i[0] (the octal MSB) on the current bit"""
    a = np.asarray(a, np.uint8)
    D = len(a)
    d = np.zeros((3, D), np.uint8)
    for i, g in enumerate(CONV_G):
        for j in range(7):
            if (g >> (6 - j)) & 1:
                d[i] ^= np.roll(a, j)
    return d


def conv_rate_match(d, Q):
    """5.1.4.2: per-stream sub-block interleaver of 32 columns (<NULL> padded in front), circular buffer w = v0 v1
    v2, the first Q non-null bits from position 0 on, wrapping"""
    D = d.shape[1]
    R = -(-D // 32)
    w = []
    for i in range(3):
        y = np.concatenate([np.full(32 * R - D, 2, np.uint8), d[i]]).reshape(R, 32)
        w.append(y[:, CONV_PERM].T.ravel())
    w = np.concatenate(w)
    w = w[w != 2]
    return w[np.arange(Q) % len(w)]


def cqi_encode(c, Q):
    """the Q coded CQI bits q_0 .. q_(Q-1)"""
    o = np.array(c.cqi[:c.cqi_len], np.uint8)
    if c.cqi_len <= 11:      # (32, O) block code, circularly repeated
        w = O.lib().or_cqi_rm32(o, c.cqi_len)
        b = np.array([(w >> (31 - i)) & 1 for i in range(32)], np.uint8)
        return b[np.arange(Q) % 32]
    crc = O.lib().or_crc(o, c.cqi_len, 0x9B, 8)              # g_CRC8 = D^8 + D^7 + D^4 + D^3 + D + 1
    a = np.concatenate([o, np.array([(crc >> (7 - i)) & 1 for i in range(8)], np.uint8)])
    return conv_rate_match(conv_encode_tb(a), Q)


# ---- UL-SCH + multiplexing (5.2.2.1-5.2.2.7) -------------------------------------------------------------
def ulsch_encode(c, tb, n_srs=0, n_symb_initial=0):
    """the multiplexed sequence g as bits: Q_CQI CQI bits, then the G rate-matched data bits"""
    L = O.lib()
    r = resource(c, n_srs, n_symb_initial)
    A, s = c.tbs, segm(c.tbs)
    b = np.unpackbits(np.asarray(tb, np.uint8))[:A]
    crc = L.or_crc24a(np.ascontiguousarray(b), A)
    b = np.concatenate([b, np.array([(crc >> (23 - i)) & 1 for i in range(24)], np.uint8)])
    out = [cqi_encode(c, r["q_cqi"] * c.Qm)] if r["q_cqi"] else []
    pos = 0
    for k, K in enumerate(cb_sizes(s)):
        F, Lc = (s.F if k == 0 else 0), (24 if s.C > 1 else 0)
        cb = np.zeros(K, np.uint8)
        cb[F:K - Lc] = b[pos:pos + K - Lc - F]
        pos += K - Lc - F
        if Lc:
            cc = L.or_crc24b(np.ascontiguousarray(cb[:K - Lc]), K - Lc)
            cb[K - Lc:] = [(cc >> (23 - i)) & 1 for i in range(24)]
        d = np.zeros(3 * (K + 4), np.uint8)
        L.or_tcod(cb, K, F, d)
        e = np.zeros(r["E"][k], np.uint8)
        L.or_rm_tx(d, K, r["E"][k], c.rv, e)
        out.append(e)
    assert pos == A + 24
    g = np.concatenate(out)
    assert len(g) == r["q_cqi"] * c.Qm + r["G"]
    return g


def symbols(c, tb, n_srs=0, n_symb_initial=0):
    """g as Qm-bit symbols (first bit = MSB), then zeros for the Q'_RI cells: the layout of mi_ul_batch_symbols"""
    g = ulsch_encode(c, tb, n_srs, n_symb_initial)
    w = (1 << np.arange(c.Qm - 1, -1, -1)).astype(np.uint32)
    s = (g.reshape(-1, c.Qm).astype(np.uint32) @ w).astype(np.uint8)
    return np.concatenate([s, np.zeros(resource(c, n_srs, n_symb_initial)["q_ri"], np.uint8)])


# ---- channel interleaver (5.2.2.8) -----------------------------------------------------------------------
def uci_cells(q, cols, M):
    """(row, column) of coded symbol i = 0 .. q - 1: from the last row up, the ColumnSet walked with j = (j + 3) mod 4"""
    i = np.arange(q)
    return M - 1 - i // 4, np.array(cols)[(3 * i) % 4]


def interleave(c, g, n_srs=0, n_symb_initial=0):
    """the interleaver matrix of M rows x C_mux = N columns of Qm-bit cells (codes 0 / 1, 2 = x, 3 = y) and, per
    cell, where its content comes from: src >= 0 the g symbol index, -1 RI, -2 HARQ-ACK.  Returns (y[M, N, Qm],
    src[M, N])"""
    r = resource(c, n_srs, n_symb_initial)
    N, M, Qm = r["n_symb"], 12 * c.L_prb, c.Qm
    y = np.zeros((M, N, Qm), np.uint8)
    src = np.full((M, N), -3, np.int64)
    blk = np.zeros(18, np.uint8)
    if r["q_ri"]:
        nb = O.lib().or_ri_block(C.byref(c), blk)
        rr, cc = uci_cells(r["q_ri"], RI_COLS, M)
        y[rr, cc] = blk[(np.arange(r["q_ri"] * Qm) % nb)].reshape(-1, Qm)
        src[rr, cc] = -1
    free = np.flatnonzero(src.ravel() == -3)                 # row by row over the cells RI left free
    assert len(free) * Qm == len(g)
    y.reshape(-1, Qm)[free] = g.reshape(-1, Qm)
    src.ravel()[free] = np.arange(len(free))
    if r["q_ack"]:                                           # HARQ-ACK overwrites (punctures) g
        nb = O.lib().or_ack_block(C.byref(c), blk)
        rr, cc = uci_cells(r["q_ack"], ACK_COLS, M)
        y[rr, cc] = blk[(np.arange(r["q_ack"] * Qm) % nb)].reshape(-1, Qm)
        src[rr, cc] = -2
    return y, src


# ---- scrambling (36.211 5.3.1), modulation (7.1) ---------------------------------------------------------
def scramble(c, h):
    cs = np.zeros(len(h), np.uint8)
    O.lib().or_gold((c.rnti << 14) | (c.sf_idx << 9) | c.cell_id, cs, len(h))
    out = np.where(h < 2, h ^ cs, 1).astype(np.uint8)        # x -> 1
    for i in np.flatnonzero(h == 3):                         # y -> the previous scrambled bit
        out[i] = out[i - 1]
    return out


def modulate(b, Qm):
    b = b.reshape(-1, Qm).astype(np.float64)
    s = 1.0 - 2.0 * b
    if Qm == 2:
        re, im, k = s[:, 0], s[:, 1], np.sqrt(2.0)
    elif Qm == 4:
        re, im, k = s[:, 0] * (2.0 - s[:, 2]), s[:, 1] * (2.0 - s[:, 3]), np.sqrt(10.0)
    else:
        re, im = s[:, 0] * (4.0 - s[:, 2] * (2.0 - s[:, 4])), s[:, 1] * (4.0 - s[:, 3] * (2.0 - s[:, 5]))
        k = np.sqrt(42.0)
    return np.stack([re / k, im / k], 1).astype(np.float32)


def mod_symbols(c, tb, n_srs=0, n_symb_initial=0):
    """x[N, M, 2]: the modulation symbols of the N data SC-FDMA symbols (column l of the interleaver = symbol l)"""
    y, _ = interleave(c, ulsch_encode(c, tb, n_srs, n_symb_initial), n_srs, n_symb_initial)
    M, N, Qm = y.shape
    h = np.ascontiguousarray(y.transpose(1, 0, 2)).ravel()   # read column by column
    return modulate(scramble(c, h), Qm).reshape(N, M, 2)


# ---- transform precoding, mapping, DMRS, SC-FDMA ---------------------------------------------------------
def grid(c, tb, n_srs=0, n_symb_initial=0):
    """float32 [14, 12 N_RB, 2]; symbol 13 stays empty when n_srs = 1"""
    L = O.lib()
    x = mod_symbols(c, tb, n_srs, n_symb_initial)
    W, M = 12 * c.nof_prb, 12 * c.L_prb
    gr = np.zeros((14, W, 2), np.float32)
    z = np.zeros(2 * M, np.float32)
    ds = 0
    for l in range(14 - n_srs):
        n0 = c.n_prb1 if (c.hop and l >= 7) else c.n_prb
        if l % 7 == 3:
            assert L.or_dmrs_pusch(C.byref(c), 2 * c.sf_idx + l // 7, z) == 0
        else:
            L.or_dft_m(np.ascontiguousarray(x[ds].ravel()), M, z, 0)
            ds += 1
        gr[l, 12 * n0:12 * n0 + M] = z.reshape(M, 2)
    assert ds == x.shape[0]
    return gr


def encode(c, tb, n_srs=0, n_symb_initial=0):
    """the subframe's SC-FDMA IQ, 2 x 15 N float32 (re, im interleaved)"""
    iq = np.zeros(2 * 15 * FFT_SIZE[c.nof_prb], np.float32)
    assert O.lib().or_scfdma_tx(c.nof_prb, np.ascontiguousarray(grid(c, tb, n_srs, n_symb_initial).ravel()), iq) == 0
    return iq


def symbol_span(nof_prb, l):
    """(first, end) complex-sample offsets of SC-FDMA symbol l (with its CP) in the subframe"""
    N = FFT_SIZE[nof_prb]
    pos = 0
    for k in range(l + 1):
        cp = (160 if k % 7 == 0 else 144) * N // 2048
        a, pos = pos, pos + N + cp
    return a, pos
