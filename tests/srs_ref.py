"""Test helper (not product code): an independent SRS transmitter and receiver (36.211 5.5.3, periodic SRS, FDD,
normal CP) in numpy over oracle primitives -- or_gold (f_gh and c(ns)), or_dmrs_pusch (the tabulated M_sc = 24 base
sequences, the trick of pucch_ref.base_seq) and or_scfdma_tx (grid to IQ).  The Zadoff-Chu base sequences are
computed here from 5.5.1.1.

resource() restates the bandwidth tables, the frequency position with hopping and the sequence parameters, vectorised
over every argument; grid() / iq() transmit; pucch_ref.demod inverts or_scfdma_tx and receive() measures a grid."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
import pucch_ref as P

NFFT = P.NFFT
# 36.211 Tables 5.5.3.2-1 .. 5.5.3.2-4: m_SRS,b by (table, b, C_SRS); written down from the specification's layout
# (one row per C_SRS: m_SRS,0, m_SRS,1, m_SRS,2, m_SRS,3) and transposed below
_ROWS = {
    0: [(36, 12, 4, 4), (32, 16, 8, 4), (24, 4, 4, 4), (20, 4, 4, 4), (16, 4, 4, 4), (12, 4, 4, 4), (8, 4, 4, 4),
        (4, 4, 4, 4)],
    1: [(48, 24, 12, 4), (48, 16, 8, 4), (40, 20, 4, 4), (36, 12, 4, 4), (32, 16, 8, 4), (24, 4, 4, 4), (20, 4, 4, 4),
        (16, 4, 4, 4)],
    2: [(72, 24, 12, 4), (64, 32, 16, 4), (60, 20, 4, 4), (48, 24, 12, 4), (48, 16, 8, 4), (40, 20, 4, 4),
        (36, 12, 4, 4), (32, 16, 8, 4)],
    3: [(96, 48, 24, 4), (96, 32, 16, 4), (80, 40, 20, 4), (72, 24, 12, 4), (64, 32, 16, 4), (60, 20, 4, 4),
        (48, 24, 12, 4), (48, 16, 8, 4)],
}
M_SRS = np.array([np.array(_ROWS[t]).T for t in range(4)], np.int64)          # [table, b, C_SRS]
# 36.213 Table 8.2-1 (FDD): first I_SRS of each row and its periodicity; 637..1023 reserved
T_ROWS = [(0, 2), (2, 5), (7, 10), (17, 20), (37, 40), (77, 80), (157, 160), (317, 320)]
I_SRS_MAX = 636


def table_of(nof_prb):
    nof_prb = np.asarray(nof_prb)
    return (nof_prb > 40).astype(np.int64) + (nof_prb > 60) + (nof_prb > 80)


def t_srs(I_srs):
    I = np.asarray(I_srs, np.int64)
    T = np.zeros_like(I)
    for first, per in T_ROWS:
        T = np.where(I >= first, per, T)
    return T


def gold(c_init, n):
    c = np.zeros(n, np.uint8)
    O.lib().or_gold(c_init, c, n)
    return c


@functools.lru_cache(maxsize=None)
def f_gh(cell_id):
    """f_gh(ns) [20] (5.5.1.3: c_init = N_ID // 30)"""
    return (gold(cell_id // 30, 160).reshape(20, 8).astype(np.int64) @ (1 << np.arange(8))) % 30


@functools.lru_cache(maxsize=None)
def c_seq(cell_id, delta_ss):
    """c(ns) [20] of sequence hopping (5.5.1.4: c_init = (N_ID // 30) 2^5 + f_ss^PUSCH)"""
    return gold((cell_id // 30) * 32 + (cell_id % 30 + delta_ss) % 30, 20).astype(np.int64)


def _is_prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


@functools.lru_cache(maxsize=None)
def n_zc(M_sc):
    return max(p for p in range(2, M_sc) if _is_prime(p))


def valid(nof_prb=6, cell_id=1, tti=0, bw_cfg=7, B=0, b_hop=3, n_rrc=0, k_tc=0, n_srs=0, I_srs=0, dss=0, **_):
    if nof_prb not in NFFT or cell_id > 503 or tti > 10239 or bw_cfg > 7 or B > 3 or b_hop > 3 or n_rrc > 23:
        return False
    if k_tc > 1 or n_srs > 7 or I_srs > I_SRS_MAX or dss > 29:
        return False
    return bool(M_SRS[table_of(nof_prb), 0, bw_cfg] <= nof_prb)


def resource(nof_prb=6, cell_id=1, tti=0, bw_cfg=7, B=0, b_hop=3, n_rrc=0, k_tc=0, n_srs=0, I_srs=0, gh=0, sh=0,
             dss=0, **_):
    """dict of int64 arrays over the broadcast of the arguments (cell_id, gh, sh, dss scalar): ok (m_SRS,0 <= nof_prb),
    m_srs, M_sc, k0, n_b [.., 4], N_b [.., 4], n_SRS, T_srs, u, v, nzc, q, n_cs"""
    nof_prb, tti, bw_cfg, B, b_hop, n_rrc, k_tc, n_srs, I_srs = np.broadcast_arrays(
        *[np.atleast_1d(np.asarray(a, np.int64)) for a in (nof_prb, tti, bw_cfg, B, b_hop, n_rrc, k_tc, n_srs, I_srs)])
    m = np.moveaxis(M_SRS[table_of(nof_prb), :, bw_cfg], -1, 0)       # [4, ...]
    N = np.ones_like(m)
    N[1:] = m[:-1] // m[1:]
    T = t_srs(I_srs)
    n_SRS = tti // T
    k0 = (nof_prb // 2 - m[0] // 2) * 12 + k_tc
    n_b = np.zeros_like(m)
    for b in range(4):
        pos = 4 * n_rrc // m[b]
        # F_b(n_SRS), 5.5.3.2: products over b' = b_hop .. b (and .. b - 1) with N_b_hop = 1
        lo = np.ones_like(T)
        for bp in range(b):
            lo = lo * np.where(bp > b_hop, N[bp], 1)
        hi = lo * N[b]
        even = (N[b] // 2) * ((n_SRS % hi) // lo) + (n_SRS % hi) // (2 * lo)
        odd = (N[b] // 2) * (n_SRS // lo)
        F = np.where(N[b] % 2 == 0, even, odd)
        hop = (b_hop < B) & (b > b_hop)
        n_b[b] = np.where(b <= B, (pos + np.where(hop, F, 0)) % N[b], 0)
        k0 = k0 + np.where(b <= B, 12 * m[b] * n_b[b], 0)
    m_srs = np.take_along_axis(m, B[None], 0)[0]
    M_sc = 6 * m_srs
    ns = 2 * (tti % 10) + 1
    u = ((f_gh(cell_id)[ns] if gh else 0) + cell_id % 30) % 30
    v = np.where(M_sc >= 72, c_seq(cell_id, dss)[ns], 0) if (sh and not gh) else np.zeros_like(ns)
    nzc = np.array([0 if M < 36 else n_zc(int(M)) for M in np.unique(M_sc)])[np.searchsorted(np.unique(M_sc), M_sc)]
    # q = floor(qbar + 1/2) + v (-1)^floor(2 qbar), qbar = N_ZC (u + 1) / 31, in integers
    q = np.where(nzc == 0, u, (2 * nzc * (u + 1) + 31) // 62 + v * (1 - 2 * ((2 * nzc * (u + 1) // 31) % 2)))
    return dict(ok=m[0] <= nof_prb, m_srs=m_srs, M_sc=M_sc, k0=k0, n_b=np.moveaxis(n_b, 0, -1), N_b=np.moveaxis(N, 0, -1),
                n_SRS=n_SRS, T_srs=T, u=u + 0 * ns, v=v, nzc=nzc, q=q, n_cs=n_srs)


@functools.lru_cache(maxsize=None)
def base_seq24(u):
    """r_u(n), n = 0..23 (Table 5.5.1.2-2): the oracle's PUSCH DMRS of two PRBs for a cell whose group is u, cyclic
    shift divided out"""
    c = O.ul_cfg(cell_id=u, nof_prb=6, sf_idx=0, n_prb=0, L_prb=2, tbs=16, Qm=2)
    r = np.zeros(48, np.float32)
    assert O.lib().or_dmrs_pusch(C.byref(c), 0, r) == 0
    a, b, ncs = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert O.lib().or_dmrs_params(C.byref(c), 0, C.byref(a), C.byref(b), C.byref(ncs)) == 0 and a.value == u
    z = r[0::2].astype(np.float64) + 1j * r[1::2]
    return z * np.exp(-2j * np.pi * ncs.value * np.arange(24) / 12)


def base_seq(M_sc, u, v):
    """rbar_{u,v}(n), n < M_sc (5.5.1.1 for M_sc >= 36, 5.5.1.2 for 24)"""
    if M_sc == 24:
        return base_seq24(int(u))
    nzc = n_zc(M_sc)
    q = (2 * nzc * (u + 1) + 31) // 62 + v * (1 - 2 * ((2 * nzc * (u + 1) // 31) % 2))
    mm = np.arange(M_sc) % nzc
    return np.exp(-1j * np.pi * ((q * mm * (mm + 1)) % (2 * nzc)) / nzc)


def seq(res, i=0):
    """r^(alpha)_{u,v}(n) of entry i of a resource()"""
    M = int(res["M_sc"][i])
    return np.exp(2j * np.pi * int(res["n_cs"][i]) * np.arange(M) / 8) * base_seq(M, int(res["u"][i]), int(res["v"][i]))


def grid(cfg):
    """the subframe's 14 x 12 N_RB resource grid (complex128), or None for a rejected configuration"""
    if not valid(**cfg):
        return None
    res = resource(**cfg)
    g = np.zeros((14, 12 * cfg["nof_prb"]), np.complex128)
    k0, M = int(res["k0"][0]), int(res["M_sc"][0])
    g[13, k0:k0 + 2 * M:2] = seq(res)
    return g


def iq(cfg):
    return P.grid_to_iq(grid(cfg), cfg["nof_prb"])


def demod(iq_f32, nof_prb):
    return P.demod(iq_f32, nof_prb)


def receive(g, cfg):
    """measure a demodulated grid: dict(p_early = power of symbols 0..12, rms = RMS of the occupied REs, leak = the
    largest magnitude of symbol 13 outside them, corr [8] = |correlation| with each cyclic shift, normalised to the
    occupied RMS, h = the complex gain against the configured shift)"""
    res = resource(**cfg)
    k0, M = int(res["k0"][0]), int(res["M_sc"][0])
    occ = np.zeros(g.shape[1], bool)
    occ[k0:k0 + 2 * M:2] = True
    y = g[13, occ]
    rms = float(np.sqrt(np.mean(np.abs(y) ** 2)))
    base = base_seq(M, int(res["u"][0]), int(res["v"][0]))
    shifts = np.exp(2j * np.pi * np.arange(8)[:, None] * np.arange(M)[None, :] / 8) * base[None, :]
    c = shifts.conj() @ y / M
    return dict(p_early=float(np.sum(np.abs(g[:13]) ** 2)), rms=rms, leak=float(np.max(np.abs(g[13, ~occ]))),
                corr=np.abs(c) / max(rms, 1e-30), h=complex(c[int(res["n_cs"][0])]))
