"""Float64 numpy reference of the antenna-combining DL control receiver (PDCCH soft bits, PHICH) and the grid-level
diversity fixture shared by test_ctrl_rx_ref.py and test_gpu_ctrl_rx.py.

REG lists, the quadruplet permutation, the scrambling sequences and the DCI coding come from the oracle
(or_pdcch_regs, or_pdcch_quad_perm, or_gold, or_dci_encode / or_dci_decode); the equalisation is the maximum-ratio
combining of the PDSCH demapper (tests/pdsch_rx_ref.py), the QPSK soft bits and the descrambling are o_ctrl.c's:
  1 port:  x = sum_a y_a h_a* / (sum_a |h_a|^2 + noise)
  2 ports: hh = sum_a (|h00_a|^2 + |h11_a|^2) (<= 0 -> 1e-9), x0 = sqrt2 sum_a (h00_a* r0_a + h11_a r1_a*) / hh,
           x1 = sqrt2 sum_a (-h10_a r0_a* + h01_a* r1_a) / hh          (h[port][RE of the pair])
Arrays: grids [n_rx, 14 W] and ces [n_rx, ports, 14 W], complex."""
import ctypes as C

import numpy as np

import oracle_lib as O

NSYMB = 14


def regs(q):
    """(re [M, 4] grid indices in 36.211 6.8.5 order, logical quadruplet of each REG [M], n_cce)"""
    n = C.c_uint32()
    M = O.lib().or_pdcch_regs(C.byref(q), None, C.byref(n))
    re = np.zeros(4 * M, np.uint32)
    O.lib().or_pdcch_regs(C.byref(q), re.ctypes.data, C.byref(n))
    lg = np.zeros(M, np.uint32)
    O.lib().or_pdcch_quad_perm(M, q.cell.id, lg)
    return re.reshape(M, 4).astype(np.int64), lg.astype(np.int64), n.value


def gold(c_init, n):
    b = np.zeros(n, np.uint8)
    O.lib().or_gold(c_init, b, n)
    return b


def equalise(grids, ces, re, noise=0.0, floor=False):
    """the equalised symbols of the REs re [..., 2 k] (2 ports: consecutive entries are SFBC pairs); floor: the one-port
    PHICH's 1e-9 floor on the summed denominator instead of the regulariser"""
    g = np.asarray(grids, np.complex128)
    h = np.asarray(ces, np.complex128)
    if h.shape[1] == 1:
        num = (g[:, re] * np.conj(h[:, 0][:, re])).sum(0)
        den = (np.abs(h[:, 0][:, re]) ** 2).sum(0)
        den = np.where(den <= 0, 1e-9, den) if floor else den + noise
        return num / den
    ra, rb = re[..., 0::2], re[..., 1::2]
    r0, r1 = g[:, ra], g[:, rb]
    h00, h01, h10, h11 = h[:, 0][:, ra], h[:, 0][:, rb], h[:, 1][:, ra], h[:, 1][:, rb]
    hh = (np.abs(h00) ** 2 + np.abs(h11) ** 2).sum(0)
    hh = np.where(hh <= 0, 1e-9, hh)
    x = np.zeros(re.shape, np.complex128)
    x[..., 0::2] = np.sqrt(2.0) * (np.conj(h00) * r0 + h11 * np.conj(r1)).sum(0) / hh
    x[..., 1::2] = np.sqrt(2.0) * (-h10 * np.conj(r0) + np.conj(h01) * r1).sum(0) / hh
    return x


def qpsk_llr(x):
    """max-log soft bits of o_ctrl.c (LLR > 0: bit 1), [..., 2]: I then Q"""
    a = 1.0 / np.sqrt(2.0)
    f = lambda v: ((v - a) ** 2 - (v + a) ** 2) / 0.5
    return np.stack([f(x.real), f(x.imag)], -1)


def pdcch_llr_rx(q, grids, ces, noise=0.0):
    """the 8 M soft bits in logical (CCE) order, descrambled, and n_cce"""
    re, lg, n_cce = regs(q)
    x = equalise(grids, ces, re, noise)                       # [M, 4]
    l = qpsk_llr(x).reshape(len(re), 8)
    out = np.zeros((len(re), 8))
    out[lg] = l
    cs = gold(q.sf * 512 + q.cell.id, 8 * len(re)).reshape(len(re), 8)
    return np.where(cs == 1, -out, out).reshape(-1), n_cce


PHICH_W = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1],
                    [1j, 1j, 1j, 1j], [1j, -1j, 1j, -1j], [1j, 1j, -1j, -1j], [1j, -1j, -1j, 1j]])   # Table 6.9.1-2


def phich_soft_rx(q, grids, ces, group, seq):
    """soft HI (> 0 favours ACK) of PHICH (group, seq): or_phich_soft's despreading over the combined symbols"""
    re = np.zeros(12, np.uint32)
    assert O.lib().or_phich_res(C.byref(q), group, re) == 0
    x = equalise(grids, ces, re.astype(np.int64), floor=True)
    cs = gold(O.lib().or_phich_cinit(q.cell.id, q.sf), 12)
    y = np.conj(PHICH_W[seq][np.arange(12) % 4]) * x
    return float(-np.sum((1.0 - 2.0 * cs) * (y.real + y.imag) / np.sqrt(2.0)))


def dci_decode(llr, ncce, L, A, rnti):
    """or_dci_decode of the candidate (L, ncce): (crc matches rnti, bits)"""
    out = np.zeros(A, np.uint8)
    e = np.ascontiguousarray(llr[72 * ncce:72 * (ncce + L)], np.float32)
    ok = O.lib().or_dci_decode(e, L, A, rnti, out.ctypes.data)
    return bool(ok), out


def search(llr, n_cce, sf, rnti, sizes):
    """The C-RNTI DL search in the order of mi_dl_ctrl_result(ul = 0): the UE-specific space with sizes[0] (the 0/1A
    size: flag bit 1) then sizes[1], then the common space with sizes[0]; every size over all candidates of a space at
    a time.  (size index, bits, L, ncce) of the first CRC match, or None."""
    Ls, nc = np.zeros(32, np.uint32), np.zeros(32, np.uint32)
    for common, idx in ((0, 0), (0, 1), (1, 0)):
        k = O.lib().or_search_space(n_cce, sf, rnti, common, Ls, nc)
        for i in range(k):
            ok, bits = dci_decode(llr, int(nc[i]), int(Ls[i]), sizes[idx], rnti)
            if ok and (idx == 1 or bits[0] == 1):
                return idx, bits, int(Ls[i]), int(nc[i])
    return None


# ---- the diversity fixture: a PDCCH that neither antenna holds alone --------------------------------------------
def pdcch_tx_grid(q, rnti, L, ncce, payload):
    """per-port transmit grids [2, 14 W] of one DCI on CCEs ncce .. ncce + L - 1 (or_tx_pdcch's mapping: QPSK, SFBC on
    each REG's RE pairs), 2 ports"""
    re, lg, n_cce = regs(q)
    W = 12 * q.cell.nof_prb
    e = np.zeros(72 * L, np.uint8)
    a = np.ascontiguousarray(payload, np.uint8)
    assert O.lib().or_dci_encode(a, len(a), rnti, L, e) == 0
    b = np.zeros(8 * len(re), np.uint8)
    b[72 * ncce:72 * (ncce + L)] = e
    b ^= gold(q.sf * 512 + q.cell.id, 8 * len(re))
    X = np.zeros((2, NSYMB * W), np.complex128)
    s2 = 1.0 / np.sqrt(2.0)
    for i in range(len(re)):
        qd = lg[i]
        if not 9 * ncce <= qd < 9 * (ncce + L):
            continue
        x = [(1 - 2 * int(b[8 * qd + 2 * j])) * s2 + 1j * (1 - 2 * int(b[8 * qd + 2 * j + 1])) * s2 for j in range(4)]
        for j in (0, 2):                                      # 36.211 6.3.4.3
            ra, rb = re[i, j], re[i, j + 1]
            X[0, ra], X[1, ra] = s2 * x[j], -s2 * np.conj(x[j + 1])
            X[0, rb], X[1, rb] = s2 * x[j + 1], s2 * np.conj(x[j])
    return X


def diversity_fixture(seed=0):
    """6 PRB, 2 ports, cfi 2, noiseless: subframe 0 carries a format 2 DCI (31 bits: a 47-bit coded block), subframe 1
    a format 2A DCI (28: 44), each on one CCE (an L = 1 candidate of its RNTI).  Antenna 0's channel is non-zero only on
    the REs of the CCE's logical quadruplets 0..3, antenna 1's only on quadruplets 4..8; grid_a = sum_p H_a[p] X[p]
    and the estimates are H_a itself, all float32-exact complex64.  Each antenna alone then holds 32 / 40 of the 72 coded
    bits of the CCE, fewer than the block.
    A list of dicts: q, rnti, fmt ('2' / '2A'), tm, A, bits, ncce, grids [2, 14 W], ces [2, 2, 14 W] (complex64)."""
    import dci2_ref as D
    rng = np.random.default_rng(0xD1F0 + seed)
    out = []
    for s, (fmt, tm) in enumerate((("2", 4), ("2A", 3))):
        q = O.ctrl_cfg(cell_id=23 + s, nof_prb=6, nof_ports=2, ng=2, cfi=2, sf=2 + 3 * s)
        rnti = 0x61 + 5 * s
        re, lg, n_cce = regs(q)
        Ls, nc = np.zeros(32, np.uint32), np.zeros(32, np.uint32)
        k = O.lib().or_search_space(n_cce, q.sf, rnti, 0, Ls, nc)
        ncce = int([nc[i] for i in range(k) if Ls[i] == 1][1])
        g = D.random_grant(rng, fmt, 6)
        bits = np.array(D.pack(6, g), np.uint8)
        X = pdcch_tx_grid(q, rnti, 1, ncce, bits)
        W = 72
        H = np.zeros((2, 2, NSYMB * W), np.complex64)
        for a, quads in enumerate((range(0, 4), range(4, 9))):
            for i in range(len(re)):
                if lg[i] - 9 * ncce in quads:
                    mag = 0.6 + 0.8 * rng.random((2, 4))
                    H[a][:, re[i]] = (mag * np.exp(2j * np.pi * rng.random((2, 4)))).astype(np.complex64)
        grids = (H.astype(np.complex128) * X[None]).sum(1).astype(np.complex64)
        out.append(dict(q=q, rnti=rnti, fmt=fmt, tm=tm, A=len(bits), bits=bits, ncce=ncce, n_cce=n_cce, grids=grids, ces=H))
    return out
