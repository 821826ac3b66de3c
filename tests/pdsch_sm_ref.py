"""Two-layer spatial multiplexing (TM3 open loop with large-delay CDD, TM4 closed loop) on top of tests/pdsch_ref.py:
float64 numpy.  2 CRS ports, 2 receive antennas, 2 layers, 2 codewords, one codeword per layer.

Spec (one right answer): per-codeword scrambling c_init = rnti 2^14 + q 2^13 + sf 2^9 + N_ID (36.211 6.3.1), the layer
mapping x0(i) = d0(i), x1(i) = d1(i) (6.3.3.2) and the precoding [y0; y1] = P_i [x0; x1] with P_i = W(i) D(i) U
(6.3.4.2.2) or the codebook matrix (6.3.4.2.3); P_i is built here from the spec's W, D(i), U definitions for v = 2,
and i is the running index of the RE in PDSCH mapping order.

Conventions (this project's receiver, extending C5 of pdsch_ref): the detector is
    x^ = (G^H G + noise I)^-1 G^H y,   G = H P_i,   H[a][p] = antenna a's estimate of port p,   noise = 0.01,
biased like the TM1 equaliser, with no per-layer SINR weighting; then C7's max-log demapper at sigma^2 = 0.5 and the
descrambling of each codeword.  Rate matching keeps C1 (N_cb = K_w: no K_MIMO halving of the softbuffer), N_L = 1."""
import functools

import numpy as np

import pdsch_ref as R
import pdsch_ref_util as U

NOISE = 0.01
PRECODERS = ((3, 0), (4, 1), (4, 2))          # (tm, pmi)

# 36.211 Table 6.3.4.2.3-1, two antenna ports, v = 2: codebook index -> matrix
CODEBOOK_2L = {0: np.array([[1, 0], [0, 1]]) / np.sqrt(2), 1: np.array([[1, 1], [1, -1]]) / 2,
               2: np.array([[1, 1], [1j, -1j]]) / 2}
# 36.211 Table 6.3.4.2.2-1, v = 2
CDD_U = np.array([[1, 1], [1, np.exp(-2j * np.pi / 2)]]) / np.sqrt(2)


def cdd_D(i):
    """D(i) of Table 6.3.4.2.2-1 for v = 2: diag(1, exp(-j 2 pi i / 2)), [n, 2, 2]"""
    i = np.asarray(i)
    D = np.zeros(i.shape + (2, 2), np.complex128)
    D[..., 0, 0] = 1
    D[..., 1, 1] = np.exp(-2j * np.pi * i / 2)
    return D


def precoder(tm, pmi, i):
    """P_i [n, 2, 2] from the spec's definitions: TM3 W(i) D(i) U with W(i) = C_1, the codebook's index 0 (two ports:
    6.3.4.2.2); TM4 the codebook's matrix of index pmi"""
    i = np.asarray(i)
    if tm == 3:
        return CODEBOOK_2L[0] @ cdd_D(i) @ CDD_U
    assert tm == 4 and pmi in (1, 2)
    return np.broadcast_to(CODEBOOK_2L[pmi], i.shape + (2, 2)).astype(np.complex128)


def precoder_closed(tm, pmi, i):
    """the closed forms the code under test implements: (1/2) [[1, 1], [w, -w]], w = (-1)^i, 1 or j"""
    i = np.asarray(i)
    w = (1.0 - 2.0 * (i % 2)) if tm == 3 else np.full(i.shape, 1.0 if pmi == 1 else 1j)
    P = np.ones(i.shape + (2, 2), np.complex128) / 2
    P[..., 1, 0] = w / 2
    P[..., 1, 1] = -w / 2
    return P


class Pair:
    """One spatially multiplexed subframe: the codewords' pdsch_ref.Cfg (own tbs, Qm, rv; everything else shared), the
    transmission mode and the TM4 codebook index."""

    def __init__(self, tm, pmi, Qm, tbs, rv=(0, 0), **kw):
        assert (tm, pmi) in PRECODERS
        self.tm, self.pmi = tm, pmi
        self.cw = [R.Cfg(nof_ports=2, tm=tm, NL=1, Qm=Qm[q], tbs=tbs[q], rv=rv[q], **kw) for q in range(2)]

    @property
    def c(self):
        return self.cw[0]

    def re_mask(self):
        return self.c.re_mask()

    @property
    def nre(self):
        return int(self.re_mask().sum())

    def abi(self, new_tb=(1, 1)):
        out = []
        for q, c in enumerate(self.cw):
            a = U.to_abi(c, new_tb=new_tb[q])
            a.cw, a.pmi = q, self.pmi
            out.append(a)
        return out


def c_init(pair, q):
    c = pair.cw[q]
    return R.pdsch_c_init(c.rnti, c.sf, c.cell_id, q)


def precode(pair, x0, x1):
    """layer symbols in mapping order -> per-port symbols y[2, n]"""
    P = precoder(pair.tm, pair.pmi, np.arange(len(x0)))
    return np.einsum("npl,nl->pn", P, np.stack([x0, x1], 1))


def put_common(c, grids):
    """CRS and PCFICH of a two-port subframe, as pdsch_ref.tx_grid places them"""
    for p in range(2):
        for l in (0, 4, 7, 11):
            r, k = R.crs(c.cell_id, 2 * c.sf + l // 7, l % 7, p, c.nof_prb)
            grids[p, l, k] = r
    y, k = R.pcfich(c.cell_id, c.nof_prb, 2, c.cfi, c.sf)
    grids[:, 0, k] = y
    return grids


def tx_grid(pair, tbs):
    """Per-port grids [2, 14, W]: both transport blocks coded (N_L = 1), scrambled per codeword, modulated, layer
    mapped and precoded onto the PDSCH REs; CRS and PCFICH"""
    mask, xs = pair.re_mask(), []
    for q, c in enumerate(pair.cw):
        f = R.dlsch_encode(c.tbs, R.bytes_to_bits(tbs[q])[:c.tbs], pair.nre * c.Qm, c.Qm, 1, c.rv, U.qpp())
        xs.append(R.modulate(R.scramble(f, c_init(pair, q)), c.Qm))
    y = precode(pair, xs[0], xs[1])
    grids = np.zeros((2, R.NSYMB, pair.c.W), np.complex128)
    grids[0][mask], grids[1][mask] = y[0], y[1]
    return put_common(pair.c, grids)


def effective_channel(pair, ces, tm=None, pmi=None):
    """G[n, antenna, layer] = H P_i on the PDSCH REs, H[n, a, p] from ces[a][p]"""
    mask = pair.re_mask()
    H = np.stack([np.stack([ce[0][mask], ce[1][mask]], 1) for ce in ces], 1)      # [n, a, p]
    tm, pmi = (pair.tm, pair.pmi) if tm is None else (tm, pmi)
    return H @ precoder(tm, pmi, np.arange(H.shape[0]))


def gram(G, noise=NOISE):
    return np.conj(np.swapaxes(G, 1, 2)) @ G + noise * np.eye(2)


def detect(pair, grids, ces, noise=NOISE, tm=None, pmi=None):
    """the layers' symbols (x0, x1) in mapping order: np.linalg.solve of (G^H G + noise I) x = G^H y per RE"""
    mask = pair.re_mask()
    G = effective_channel(pair, ces, tm, pmi)
    y = np.stack([g[mask] for g in grids], 1)[:, :, None]                         # [n, a, 1]
    x = np.linalg.solve(gram(G, noise), np.conj(np.swapaxes(G, 1, 2)) @ y)[:, :, 0]
    return x[:, 0], x[:, 1]


def pdsch_llr_sm(pair, grids, ces, noise=NOISE, tm=None, pmi=None, swap_q=False):
    """(llr of codeword 0, of codeword 1).  tm / pmi: detect as another precoder; swap_q: descramble codeword q with
    the other one's sequence -- both must break the decode (the tests use them to show the check can fail)"""
    xs = detect(pair, grids, ces, noise, tm, pmi)
    return [R.descramble(R.demap(xs[q], pair.cw[q].Qm), c_init(pair, q ^ int(swap_q))) for q in range(2)]


def decode(pair, llrs, soft=(None, None), n_its=8):
    """per codeword (crc ok, payload, soft)"""
    return [R.dlsch_decode(pair.cw[q], llrs[q], U.qpp(), soft[q], n_its=n_its) for q in range(2)]


# ---- detector inputs shared by the CPU emulation test and the GPU demap test -------------------------------------------
DETECT_TABLE = [
    # nof_prb, Qm0, Qm1, (tm, pmi), sf, cfi, cell_id
    (6, 2, 6, (3, 0), 1, 1, 30),
    (6, 4, 4, (4, 1), 0, 1, 31),
    (6, 6, 2, (4, 2), 5, 3, 32),
    (15, 6, 6, (3, 0), 3, 2, 33),
    (15, 4, 6, (4, 2), 7, 1, 34),
    (100, 6, 6, (3, 0), 1, 1, 35),
    (100, 6, 4, (4, 1), 2, 3, 36),
    (25, 2, 2, (3, 0), 9, 2, 37),
]
DET_MIN = 5e-3      # the inputs keep det(G^H G + noise I) at or above this on every RE


@functools.lru_cache(None)
def detect_pairs():
    """the table's eight pairs, then the distributed allocation of test_gpu_pdsch_ref.demap_cfgs() (TM3, Qm 4 / 6)"""
    from test_gpu_pdsch_ref import demap_cfgs
    out = [Pair(tm, pmi, (q0, q1), (104, 104), cell_id=cid, nof_prb=nprb, sf=sf, cfi=cfi, rnti=0x300 + j)
           for j, (nprb, q0, q1, (tm, pmi), sf, cfi, cid) in enumerate(DETECT_TABLE)]
    d = demap_cfgs()[-1]
    assert not np.array_equal(d.prb_slots[0], d.prb_slots[1])
    out.append(Pair(3, 0, (4, 6), (104, 104), cell_id=d.cell_id, nof_prb=d.nof_prb, sf=d.sf, cfi=d.cfi, rnti=0x300 + len(out),
                    prb_slots=d.prb_slots))
    return tuple(out)


def symbol_grid(pair, seed):
    """per-port grids holding random modulation symbols of both layers, precoded, on the PDSCH REs only"""
    rng = np.random.default_rng(0x5B0 + seed)
    xs = [R.modulate(rng.integers(0, 2, pair.nre * c.Qm), c.Qm) for c in pair.cw]
    y = precode(pair, xs[0], xs[1])
    g = np.zeros((2, R.NSYMB, pair.c.W), np.complex128)
    g[0][pair.re_mask()], g[1][pair.re_mask()] = y[0], y[1]
    return g


@functools.lru_cache(None)
def detect_inputs():
    """per pair j: (float32 interleaved grids [2][14 W], estimates [2][2 14 W]) of two antennas seeing the pair's
    symbols through U.channel(c, 20 + j + 500 a) at 25 dB with exactly known estimates, and the lowest
    det(G^H G + noise I) over all pairs (asserted >= DET_MIN)"""
    out, lowest = [], np.inf
    for j, p in enumerate(detect_pairs()):
        Hs = [U.channel(p.c, 20 + j + 500 * a) for a in range(2)]
        det = np.linalg.det(gram(effective_channel(p, Hs))).real
        assert det.min() >= DET_MIN, (j, det.min())
        lowest = min(lowest, float(det.min()))
        X = symbol_grid(p, j)
        out.append(([U.f32c(U.rx_grid(X, H, 25.0, j + 500 * a)) for a, H in enumerate(Hs)], [U.f32c(H) for H in Hs]))
    return tuple(out), lowest


def as_grids(pair, g32s):
    return [U.c128(g).reshape(R.NSYMB, pair.c.W) for g in g32s]


def as_ces(pair, c32s):
    return [U.c128(c).reshape(2, R.NSYMB, pair.c.W) for c in c32s]


# ---- the end-to-end scenario (CPU test 4 pins it, the emulated chain and the GPU test run it) --------------------------
E2E_SEEDS = tuple(range(6))
E2E_SNR_DB = 30.0
E2E_MCS = ((4, 1000, 6, 1544), (2, 504, 6, 1544), (6, 1544, 6, 1544))     # (Qm0, tbs0, Qm1, tbs1)


def e2e_pair(seed, prec, mcs, rv=(0, 0)):
    return Pair(prec[0], prec[1], (mcs[0], mcs[2]), (mcs[1], mcs[3]), rv=rv, cell_id=7 + seed, nof_prb=6, sf=1, cfi=1)


@functools.lru_cache(None)
def e2e_samples(seed, prec, mcs, snr_db=E2E_SNR_DB, rv=(0, 0), tb_seed=None):
    """(pair, [tb0, tb1], [complex128 samples of antenna 0, of antenna 1]): one transmit grid through each antenna's
    channel U.channel(cfg, 100 seed + a), each antenna with its own noise"""
    pair = e2e_pair(seed, prec, mcs, rv)
    k = PRECODERS.index(prec)
    t0 = 1200 + 20 * seed + 2 * k if tb_seed is None else tb_seed
    tbs = [U.tb_bytes(t0 + q, pair.cw[q].tbs) for q in range(2)]
    grids = tx_grid(pair, tbs)
    rv_tag = 4 * rv[0] + rv[1]
    iqs = [R.ofdm_tx(grids, U.channel(pair.c, 100 * seed + a), snr_db,
                     np.random.default_rng(0x5A700 + 1000 * rv_tag + 100 * k + 10 * seed + a)) for a in range(2)]
    return pair, tbs, iqs


def front(pair, iqs):
    """reference front end per antenna: (grids, ces)"""
    grids = [R.ofdm_rx(iq, pair.c.nof_prb) for iq in iqs]
    return grids, [R.chest(g, pair.c.cell_id, pair.c.nof_prb, 2, pair.c.sf)[0] for g in grids]


# ---- the HARQ scenario: codeword 1 at rv 0, then rv 2 (new_tb = 0); codeword 0 a new transport block both times --------
HARQ_PREC = (3, 0)
HARQ_MCS = (4, 1000, 6, 1544)
HARQ_SNR_DB = 21.5      # chosen with the reference: codeword 1 fails alone and passes combined (test_pdsch_sm_ref.py pins it)
HARQ_SEED = 0


def harq_samples():
    """[(pair, tbs, iqs) of transmission 0, of transmission 1]: codeword 1 carries one transport block at rv 0 then rv 2,
    codeword 0 a different new one each time"""
    first = e2e_samples(HARQ_SEED, HARQ_PREC, HARQ_MCS, HARQ_SNR_DB, (0, 0), 1900)
    # transmission 1: tb seeds 1902 (cw 0, new) and 1901 (cw 1, the same block again)
    pair = e2e_pair(HARQ_SEED, HARQ_PREC, HARQ_MCS, (0, 2))
    tbs = [U.tb_bytes(1902, pair.cw[0].tbs), first[1][1]]
    grids = tx_grid(pair, tbs)
    iqs = [R.ofdm_tx(grids, U.channel(pair.c, 100 * HARQ_SEED + a), HARQ_SNR_DB, np.random.default_rng(0x5A7F0 + a))
           for a in range(2)]
    return [first, (pair, tbs, iqs)]
