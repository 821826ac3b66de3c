"""Test helper (not product code): an independent PUCCH transmitter and receiver (36.211 5.4, 5.5.2.2; formats
1/1a/1b and 2/2a/2b, normal CP) in numpy over oracle primitives -- or_gold (every pseudo-random sequence),
or_dmrs_pusch / or_dmrs_params (the M_sc = 12 base sequences), or_cqi_rm32 (the (20, A) code is its top 20 bits)
and or_scfdma_tx (grid to IQ).

resource() restates the resource derivation, vectorised over n_pucch; grid() / iq() transmit; demod() inverts
or_scfdma_tx and receive() recovers the HARQ-ACK and CQI bits from a grid."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O

F1, F1A, F1B, F2, F2A, F2B = range(6)
NFFT = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}
DATA_1, DMRS_1 = (0, 1, 5, 6), (2, 3, 4)      # formats 1x: symbols of a slot
DATA_2, DMRS_2 = (0, 2, 3, 4, 6), (1, 5)      # formats 2x
W4 = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, -1, -1, 1]], np.complex128)
OM = np.exp(2j * np.pi / 3)
W3 = np.array([[1, 1, 1], [1, OM, OM ** 2], [1, OM ** 2, OM]])
D_1B = {(0, 0): 1, (0, 1): -1j, (1, 0): 1j, (1, 1): -1}      # 36.211 Table 5.4.1-1 (b(0), b(1))


def gold(c_init, n):
    c = np.zeros(n, np.uint8)
    O.lib().or_gold(c_init, c, n)
    return c


@functools.lru_cache(maxsize=None)
def cell_shifts(cell_id):
    """n_cs^cell(ns, l) [20, 7] (5.4: c_init = N_ID) and f_gh(ns) [20] (5.5.1.3: c_init = N_ID // 30)"""
    w = 1 << np.arange(8)
    ncs = gold(cell_id, 8 * 7 * 20).reshape(20, 7, 8).astype(np.int64) @ w
    fgh = (gold(cell_id // 30, 8 * 20).reshape(20, 8).astype(np.int64) @ w) % 30
    return ncs, fgh


@functools.lru_cache(maxsize=None)
def base_seq(u):
    """r_u(n), n = 0..11: the oracle's PUSCH DMRS of one PRB for a cell whose group is u, cyclic shift divided out"""
    c = O.ul_cfg(cell_id=u, nof_prb=6, sf_idx=0, n_prb=0, L_prb=1, tbs=16, Qm=2)
    r = np.zeros(24, np.float32)
    assert O.lib().or_dmrs_pusch(C.byref(c), 0, r) == 0
    a, b, ncs = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert O.lib().or_dmrs_params(C.byref(c), 0, C.byref(a), C.byref(b), C.byref(ncs)) == 0 and a.value == u
    z = r[0::2].astype(np.float64) + 1j * r[1::2]
    return z * np.exp(-2j * np.pi * ncs.value * np.arange(12) / 12)


def valid(nof_prb=6, fmt=F1A, delta=1, N_cs=0, shortened=0, cqi_len=0, **_):
    """the field checks that do not depend on n_pucch"""
    if nof_prb not in NFFT or not 1 <= delta <= 3 or N_cs > 7 or N_cs % delta:
        return False
    if fmt >= F2 and (shortened or not 1 <= cqi_len <= 11):
        return False
    return True


def resource(cell_id=1, nof_prb=6, sf_idx=0, fmt=F1A, n_pucch=0, delta=1, N_cs=0, n_rb_2=0, gh=0, **_):
    """dict of arrays over n_pucch (scalar or array): ok (m < nof_prb), m, n_prb [.., 2], u [2], n_prime [.., 2],
    n_oc [.., 2], n_cs [.., 2, 7]"""
    n = np.atleast_1d(np.asarray(n_pucch, np.int64))
    c, d = 3, 2
    if fmt >= F2:
        own = n < 12 * n_rb_2
        n0 = np.where(own, n % 12, (n + N_cs + 1) % 12)
        n1 = np.where(own, (12 * (n0 + 1)) % 13 - 1, (12 - 2 - n) % 12)
        m = n // 12
        npr = np.stack([n0, n1], -1)
        noc = np.zeros_like(npr)
        off = npr
    else:
        T, per = c * N_cs // delta, c * 12 // delta
        mixed = n < T
        Np = np.where(mixed, N_cs, 12)
        Npd = np.maximum(Np, 1)      # N_cs = 0: no n is mixed
        n0 = np.where(mixed, n, (n - T) % per)
        h = (n0 + d) % np.maximum(c * Np // delta, 1)
        n1 = np.where(mixed, h // c + (h % c) * Np // delta, (c * (n0 + 1)) % (per + 1) - 1)
        m = np.where(mixed, n_rb_2, (n - T) // per + n_rb_2 + -(-N_cs // 8))
        npr = np.stack([n0, n1], -1)
        noc = npr * delta // Npd[:, None]
        off = (npr * delta + noc % delta) % Npd[:, None]
    ncs_cell, fgh = cell_shifts(cell_id)
    ns = 2 * sf_idx + np.arange(2)
    n_cs = (ncs_cell[ns][None, :, :] + off[:, :, None]) % 12
    u = ((fgh[ns] if gh else 0) + cell_id % 30) % 30
    par = (m[:, None] + np.arange(2)[None, :]) % 2
    n_prb = np.where(par == 0, m[:, None] // 2, nof_prb - 1 - m[:, None] // 2)
    return dict(ok=m < nof_prb, m=m, n_prb=n_prb, u=np.broadcast_to(u, (2,)), n_prime=npr, n_oc=noc, n_cs=n_cs)


def cqi_code(cqi):
    """b(0..19) of the (20, A) code: the first 20 bits of the oracle's (32, O) code word"""
    o = np.ascontiguousarray(list(cqi) + [0] * (11 - len(cqi)), np.uint8)
    w = O.lib().or_cqi_rm32(o, len(cqi))
    return np.array([(w >> (31 - i)) & 1 for i in range(20)], np.uint8)


def scr20(cell_id, sf_idx, rnti):
    return gold((sf_idx + 1) * (2 * cell_id + 1) * 65536 + rnti, 20)


def qpsk(b):
    b = np.asarray(b, np.float64).reshape(-1, 2)
    return ((1 - 2 * b[:, 0]) + 1j * (1 - 2 * b[:, 1])) / np.sqrt(2)


def d_ack(two_bits, ack):
    b0, b1 = ack & 1, (ack >> 1) & 1
    return D_1B[(b0, b1)] if two_bits else (1 - 2 * b0)


def symbol_factors(cfg, res, ack=0, cqi=()):
    """[2, 7] complex: what multiplies r_u^alpha(n) in each symbol (0 = nothing sent); res: scalar resource()"""
    fmt = cfg.get("fmt", F1A)
    f = np.zeros((2, 7), np.complex128)
    if fmt < F2:
        d0 = 1 if fmt == F1 else d_ack(fmt == F1B, ack)
        for s in range(2):
            noc, S = int(res["n_oc"][0, s]), (1j if res["n_prime"][0, s] % 2 else 1)
            short = cfg.get("shortened", 0) and s == 1
            for m, l in enumerate(DATA_1):
                if short:
                    f[s, l] = 0 if m == 3 else S * W3[noc, m] * d0
                else:
                    f[s, l] = S * W4[noc, m] * d0
            for m, l in enumerate(DMRS_1):
                f[s, l] = W3[noc, m]
    else:
        b = cqi_code(cqi) ^ scr20(cfg.get("cell_id", 1), cfg.get("sf_idx", 0), cfg.get("rnti", 0x46))
        d = qpsk(b)
        for s in range(2):
            for i, l in enumerate(DATA_2):
                f[s, l] = d[5 * s + i]
            f[s, 1] = 1
            f[s, 5] = 1 if fmt == F2 else d_ack(fmt == F2B, ack)
    return f


def seqs(res):
    """[2, 7, 12]: r_u^alpha(n) of every symbol"""
    n = np.arange(12)
    return np.stack([base_seq(int(res["u"][s]))[None, :] *
                     np.exp(2j * np.pi * res["n_cs"][0, s][:, None] * n[None, :] / 12) for s in range(2)])


def grid(cfg, ack=0, cqi=()):
    """the subframe's 14 x 12 N_RB resource grid (complex128), or None for a rejected configuration"""
    res = resource(**cfg)
    if not valid(**cfg) or not res["ok"][0]:
        return None
    W = 12 * cfg.get("nof_prb", 6)
    g = np.zeros((14, W), np.complex128)
    f, r = symbol_factors(cfg, res, ack, cqi), seqs(res)
    for s in range(2):
        k = 12 * int(res["n_prb"][0, s])
        g[7 * s:7 * s + 7, k:k + 12] = f[s][:, None] * r[s]
    return g


def grid_to_iq(g, nof_prb):
    x = np.stack([g.real, g.imag], -1).astype(np.float32).ravel()
    iq = np.zeros(2 * 15 * NFFT[nof_prb], np.float32)
    assert O.lib().or_scfdma_tx(nof_prb, x, iq) == 0
    return iq


def iq(cfg, ack=0, cqi=()):
    return grid_to_iq(grid(cfg, ack, cqi), cfg.get("nof_prb", 6))


def demod(iq_f32, nof_prb):
    """inverse of or_scfdma_tx: drop the CP, undo the half-subcarrier shift, DFT; 14 x 12 N_RB complex grid"""
    N, W = NFFT[nof_prb], 12 * nof_prb
    z = np.asarray(iq_f32, np.float64).reshape(-1, 2)
    z = z[:, 0] + 1j * z[:, 1]
    n = np.arange(N)
    bins = (np.arange(W) - W // 2) % N
    g, pos = np.zeros((14, W), np.complex128), 0
    for l in range(14):
        pos += (160 if l % 7 == 0 else 144) * N // 2048
        X = np.fft.fft(z[pos:pos + N] * np.exp(-1j * np.pi * n / N)) / np.sqrt(N)
        g[l] = X[bins]
        pos += N
    return g


def slot_vectors(g, cfg):
    """[2][data, dmrs]: the slot's data / DMRS REs on the resource's PRB as flat vectors (orthogonality checks)"""
    res = resource(**cfg)
    dat, ref = (DATA_1, DMRS_1) if cfg.get("fmt", F1A) < F2 else (DATA_2, DMRS_2)
    out = []
    for s in range(2):
        k = 12 * int(res["n_prb"][0, s])
        blk = g[7 * s:7 * s + 7, k:k + 12]
        out.append((blk[list(dat)].ravel(), blk[list(ref)].ravel()))
    return out


def receive(g, cfg):
    """(ack, cqi bits) from a grid: correlate every symbol with its sequence, the DMRS give the channel, decide
    d(0) / d(10) on the constellation and, for formats 2x, the maximum-likelihood code word over all 2^A"""
    fmt = cfg.get("fmt", F1A)
    res = resource(**cfg)
    r = seqs(res)
    y = np.zeros((2, 7), np.complex128)
    for s in range(2):
        k = 12 * int(res["n_prb"][0, s])
        y[s] = np.sum(g[7 * s:7 * s + 7, k:k + 12] * np.conj(r[s]), -1) / 12

    def decide(z, two_bits):
        cands = [(a, d_ack(two_bits, a)) for a in range(4 if two_bits else 2)]
        return min(cands, key=lambda t: abs(z - t[1]))[0]

    if fmt < F2:
        f = symbol_factors(cfg, res, 0, ())       # covers and S with d(0) = 1
        z = 0
        for s in range(2):
            h = np.mean(y[s, list(DMRS_1)] * np.conj(f[s, list(DMRS_1)]))
            used = [l for l in DATA_1 if f[s, l] != 0]
            z += np.mean(y[s, used] * np.conj(f[s, used])) / h / 2
        return (0 if fmt == F1 else decide(z, fmt == F1B)), []
    h = y[:, 1]
    ack = 0 if fmt == F2 else decide(np.mean(y[:, 5] / h), fmt == F2B)
    d = np.concatenate([y[s, list(DATA_2)] / h[s] for s in range(2)])
    A = cfg["cqi_len"]
    scr = scr20(cfg.get("cell_id", 1), cfg.get("sf_idx", 0), cfg.get("rnti", 0x46))
    # the code is linear: all 2^A code words from the A unit messages
    cols = np.stack([cqi_code([0] * k + [1]) for k in range(A)]).astype(np.int64)
    msgs = (np.arange(1 << A)[:, None] >> np.arange(A)[None, :]) & 1
    book = ((msgs @ cols) % 2).astype(np.uint8) ^ scr[None, :]
    sym = ((1 - 2.0 * book[:, 0::2]) + 1j * (1 - 2.0 * book[:, 1::2])) / np.sqrt(2)
    best = int(np.argmax(np.real(sym.conj() @ d)))
    return ack, msgs[best].tolist()
