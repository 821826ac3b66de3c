"""CSI feedback (CQI / PMI / RI) from channel estimates: the float64 numpy reference of csi_kernel / emu_csi.

Definitions (project conventions, DESIGN.md 10 and include/mi_dl.h).  Sample points: every subcarrier of the CRS symbols
0, 4, 7, 11.  H[a][p] = antenna a's estimate of port p, n = the subframe's noise.  Per-layer SINR g at a point:
    BASE       one port: sum_a |h_a0|^2 / n;  two ports: sum |H|^2 / (2 n)
    R1 + i     rank 1, codebook index i of 36.211 Table 6.3.4.2.3-1 (v = 1): g = |H W_i|^2 / n
    R2 + 0/1   rank 2, codebook index 1 / 2: G = H P, g_l = 1 / [(I + G^H G / n)^-1]_ll - 1
    CDD        rank 2 open loop: the TM3 precoder W D(i) U at point i of the RE order (rows in time order, subcarriers
               ascending); the two layers' capacities under that alternation, averaged -- a codeword's REs fall on both
               parities alike, so both layers report the average
cap[band][h][layer] = mean over the band's points of log2(1 + g); cqi = the CQI of 10 log10(2^cap - 1).

Kept structurally apart from the code under test: the precoders are the spec's matrices (pdsch_sm_ref), the rank-2 SINR
goes through numpy's matrix inverse (no closed form), CDD alternates the precoder point by point (no identity), and the
subbands come from the table."""
import functools

import numpy as np

import pdsch_ref as R
import pdsch_ref_util as U
import pdsch_sm_ref as S
from helpers import rel_err

NHYP, MAX_SB = 8, 14
H_BASE, H_R1, H_CDD, H_R2 = 0, 1, 5, 6
PILOT_ROWS = (0, 4, 7, 11)
TOL = 1e-4                 # the project's float tolerance (helpers.rel_err)
CQI_GUARD_DB = 0.01        # a CQI cell whose reference SINR lies this close to a threshold is not compared ...
CQI_GUARD_SHARE = 0.05     # ... and at most this share of a test's cells may be left out
MARGIN = 1e-3              # least relative winning margin of every decision of a test case

# 36.211 Table 6.3.4.2.3-1, two antenna ports, v = 1: codebook index -> [2, 1]
CODEBOOK_1L = tuple(np.array([[1], [q]]) / np.sqrt(2) for q in (1, -1, 1j, -1j))
# 36.213 Table 7.2.1-3: system bandwidth (PRB, inclusive) -> subband size k; below 8 PRB no subbands
SUBBAND_TABLE = ((8, 26, 4), (27, 63, 6), (64, 110, 8))
# the SNR (dB) thresholds of srslte_cqi_from_snr: CQI = how many the SNR reaches
CQI_THR = np.array([1.95, 4.0, 6.0, 8.0, 10.0, 11.95, 14.05, 16.0, 17.9, 19.9, 21.5, 23.45, 25.0, 27.3, 29.0])


def subbands(nof_prb):
    """(subband size in PRB, number of subbands); the last subband holds the remaining PRBs"""
    for lo, hi, k in SUBBAND_TABLE:
        if lo <= nof_prb <= hi:
            return k, int(np.ceil(nof_prb / k))
    return 0, 0


def bands(nof_prb):
    """subcarrier ranges of band 0 (everything) and of the subbands"""
    k, n = subbands(nof_prb)
    return [(0, 12 * nof_prb)] + [(12 * k * b, min(12 * k * (b + 1), 12 * nof_prb)) for b in range(n)]


def points(ces, compact=False):
    """H[row, k, antenna, port] of the four pilot rows from ces[antenna][port][14 or 4][W]"""
    ces = np.asarray(ces, np.complex128)
    rows = range(4) if compact else PILOT_ROWS
    return np.stack([ces[:, :, r, :] for r in rows]).transpose(0, 3, 1, 2)


def sinr_rank2(H, P, n):
    """per-layer MMSE SINR [..., 2] of G = H P through the matrix inverse"""
    G = H @ P
    A = np.eye(2) + np.conj(np.swapaxes(G, -1, -2)) @ G / n
    Ainv = np.linalg.inv(A)
    return 1.0 / np.stack([Ainv[..., 0, 0].real, Ainv[..., 1, 1].real], -1) - 1.0


def sinr_rank2_closed(H, P, n):
    """the closed 2 x 2 form, g_0 = (a d - |b|^2) / d - 1 and g_1 = (a d - |b|^2) / a - 1 with A = [[a, b], [b*, d]]"""
    G = H @ P
    A = np.eye(2) + np.conj(np.swapaxes(G, -1, -2)) @ G / n
    a, d, b = A[..., 0, 0].real, A[..., 1, 1].real, A[..., 0, 1]
    det = a * d - np.abs(b) ** 2
    return np.stack([det / d - 1, det / a - 1], -1)


def point_log2(H, n):
    """log2(1 + g) per point: lg[row, k, hypothesis, layer] (CDD: the alternating precoder's two layers), and which
    hypotheses the antenna / port counts allow"""
    n_rx, ports = H.shape[2:]
    lg = np.zeros(H.shape[:2] + (NHYP, 2))
    valid = [H_BASE]
    lg[..., H_BASE, 0] = np.log2(1 + (np.abs(H) ** 2).sum((2, 3)) / (ports * n))
    if ports == 2:
        for i, Wi in enumerate(CODEBOOK_1L):
            lg[..., H_R1 + i, 0] = np.log2(1 + (np.abs(H @ Wi) ** 2).sum((2, 3)) / n)
            valid.append(H_R1 + i)
        if n_rx == 2:
            for j, pmi in enumerate((1, 2)):
                lg[..., H_R2 + j, :] = np.log2(1 + sinr_rank2(H, S.CODEBOOK_2L[pmi], n))
                valid.append(H_R2 + j)
            i = np.arange(H.shape[0] * H.shape[1]).reshape(H.shape[:2])        # RE order: row by row
            lg[..., H_CDD, :] = np.log2(1 + sinr_rank2(H, S.precoder(3, 0, i), n))
            valid.append(H_CDD)
    return lg, sorted(valid)


def margin(best, second):
    return abs(best - second) / max(abs(best), abs(second), 1e-300)


def csi(ces, noise, nof_prb, compact=False):
    """The record of one subframe: dict of cap / cqi / snr_db / evaluated [15, 8, 2], the scalars, and `margins`, the
    relative winning margin of each decision taken."""
    H = points(ces, compact)
    n = max(float(noise), 1e-9)
    n_rx, ports = H.shape[2:]
    lg, valid = point_log2(H, n)
    k, n_sb = subbands(nof_prb)
    cap = np.zeros((1 + MAX_SB, NHYP, 2))
    ev = np.zeros(cap.shape, bool)
    for b, (k0, k1) in enumerate(bands(nof_prb)):
        m = lg[:, k0:k1].mean((0, 1))
        m[H_CDD, :] = m[H_CDD, :].mean()           # both layers: the average over the alternation
        cap[b] = m
        for h in valid:
            ev[b, h, 0] = True
            ev[b, h, 1] = h >= H_CDD
    with np.errstate(divide="ignore"):
        snr_db = np.where(cap > 0, 10 * np.log10(np.maximum(2.0 ** cap - 1, 1e-300)), -np.inf)
    cqi = (snr_db[..., None] >= CQI_THR).sum(-1).astype(np.uint8)
    out = dict(cap=cap, cqi=cqi, snr_db=snr_db, evaluated=ev, n_sb=n_sb, sb_prb=k, noise=n,
               valid_mask=sum(1 << h for h in valid), pmi_r1=0, cb_r2=0, ri_cl=1, ri_ol=1, margins={},
               cdd_layers=lg[..., H_CDD, :].mean((0, 1)))
    if ports == 2:
        r1 = cap[0, H_R1:H_R1 + 4, 0]
        order = np.argsort(-r1, kind="stable")
        out["pmi_r1"] = int(order[0])
        out["margins"]["pmi_r1"] = margin(r1[order[0]], r1[order[1]])
        if n_rx == 2:
            r2 = cap[0, H_R2:H_R2 + 2].sum(-1)
            out["cb_r2"] = 2 if r2[1] > r2[0] else 1
            out["margins"]["cb_r2"] = margin(r2[0], r2[1])
            out["ri_cl"] = 2 if r2.max() > r1.max() else 1
            out["margins"]["ri_cl"] = margin(r2.max(), r1.max())
            out["ri_ol"] = 2 if 2 * cap[0, H_CDD, 0] > cap[0, H_BASE, 0] else 1
            out["margins"]["ri_ol"] = margin(2 * cap[0, H_CDD, 0], cap[0, H_BASE, 0])
    return out


# ---- comparing a record of the code under test (abi.CsiResult) with the reference ---------------------------------------
def compare(got, want, tag, decisions=True):
    """cap at TOL, valid_mask / n_sb / sb_prb and the zero cells exact, the decisions equal (their margins are pinned
    by the CPU test), CQI equal outside the guard.  Returns (capacity rel_err, CQI cells left out, CQI cells compared or
    left out)."""
    cap, cqi = got.cap_array().astype(np.float64), got.cqi_array()
    assert (got.valid_mask, got.n_sb, got.sb_prb) == (want["valid_mask"], want["n_sb"], want["sb_prb"]), tag
    assert not cap[~want["evaluated"]].any() and not cqi[~want["evaluated"]].any(), tag
    e = rel_err(cap, want["cap"])
    assert e < TOL, (tag, e)
    if decisions:
        for k in ("pmi_r1", "cb_r2", "ri_cl", "ri_ol"):
            assert getattr(got, k) == want[k], (tag, k, getattr(got, k), want[k], want["margins"])
    ev = want["evaluated"]
    near = np.abs(want["snr_db"][..., None] - CQI_THR).min(-1) < CQI_GUARD_DB
    check = ev & ~near
    assert np.array_equal(cqi[check], want["cqi"][check]), (tag, np.argwhere(check & (cqi != want["cqi"])))
    return e, int((ev & near).sum()), int(ev.sum())


# ---- test channels ------------------------------------------------------------------------------------------------------
def selective(nof_prb, ports, n_rx, seed):
    """ces[antenna][port][14][W]: an independent selective channel (pdsch_ref_util.channel) per antenna"""
    c = R.Cfg(nof_prb=nof_prb, nof_ports=ports, tbs=104, Qm=2)
    return np.stack([U.channel(c, 7000 + 10 * seed + a) for a in range(n_rx)])


def rank_deficient(nof_prb, seed):
    """two antennas, two ports, rank one at every point: antenna 1 sees antenna 0's channel times one complex gain"""
    H = selective(nof_prb, 2, 1, seed)
    return np.concatenate([H, (0.6 - 0.7j) * H])


def as_f32(ces):
    """what the code under test is fed (interleaved float32) and exactly that as complex128 for the reference"""
    f = U.f32c(ces)
    return f, U.c128(f).reshape(np.shape(ces))


# (name, nof_prb, ports, antennas, channel seed, SNR dB, kind); the seeds are chosen so that every decision's margin is
# at least MARGIN (test_csi_ref.py asserts it for every case)
# (seed 4, the next in line for 6 PRB at 30 dB, left two rank-1 precoders 3e-5 apart: 15 of the 16 seeds tried passed)
CASES = tuple([(f"sel_{prb}prb_{snr}dB", prb, 2, 2, 24 if (prb, snr) == (6, 30) else 3 * j + i, float(snr), "selective")
               for j, prb in enumerate((6, 15, 100)) for i, snr in enumerate((0, 7, 14, 22, 30))] +
              [("rank_deficient_15prb", 15, 2, 2, 40, 20.0, "rank1"),
               ("one_port_two_rx_25prb", 25, 1, 2, 41, 12.0, "selective"),
               ("one_port_one_rx_6prb", 6, 1, 1, 42, 9.0, "selective"),
               ("two_ports_one_rx_15prb", 15, 2, 1, 43, 16.0, "selective")])


@functools.lru_cache(None)
def case(name):
    """(nof_prb, ports, n_rx, float32 estimates, noise, reference record) of CASES[name]"""
    _, prb, ports, n_rx, seed, snr, kind = next(c for c in CASES if c[0] == name)
    ces = rank_deficient(prb, seed) if kind == "rank1" else selective(prb, ports, n_rx, seed)
    f, c = as_f32(ces)
    noise = float(np.float32(10 ** (-snr / 10)))
    return prb, ports, n_rx, f, noise, csi(c, noise, prb)


# ---- the GPU tests' inputs (their decision margins are pinned by test_csi_ref.py, like those of CASES) --------------------
# uploaded estimates: (nof_prb, ports, channel seed, SNR dB) per physical subframe of a two-antenna and of a
# single-antenna batch; UPLOAD_PAIR of the two-antenna one is a TM3 codeword pair (two entries, one record)
UPLOAD = {2: ((6, 2, 60, 18.0), (15, 2, 61, 5.0), (15, 2, 62, 26.0), (25, 2, 63, 11.0), (25, 1, 64, 8.0),
              (100, 2, 65, 21.0)),
          1: ((6, 1, 66, 13.0), (15, 2, 67, 19.0))}
UPLOAD_PAIR = 2


@functools.lru_cache(None)
def upload_case(n_rx, j):
    """(float32 estimates [antenna][ports 14 W 2], noise, reference record) of UPLOAD[n_rx][j]"""
    prb, ports, seed, snr = UPLOAD[n_rx][j]
    f, c = as_f32(selective(prb, ports, n_rx, seed))
    noise = float(np.float32(10 ** (-snr / 10)))
    return f.reshape(n_rx, -1), noise, csi(c, noise, prb)


# from IQ: the spatial-multiplexing reference's 6 PRB samples, (seed, precoder, SNR dB)
IQ_CASES = ((0, (3, 0), 30.0), (1, (4, 1), 12.0), (2, (4, 2), 21.0))


def iq_case(j):
    seed, prec, snr = IQ_CASES[j]
    return S.e2e_samples(seed, prec, S.E2E_MCS[0], snr)


def mean_noise(metric_rows):
    """the noise of a subframe from its per-antenna chest metrics rows [antenna][5]"""
    return max(float(np.mean([m[3] for m in metric_rows])), 1e-9)


@functools.lru_cache(None)
def iq_case_reference_front(j):
    """the record the reference front end (float32 samples in) leads to: what the margins of the IQ cases are pinned on"""
    pair, _, iqs = iq_case(j)
    c = pair.c
    grids = [R.ofdm_rx(U.c128(U.f32c(iq)), c.nof_prb) for iq in iqs]
    est = [R.chest(g, c.cell_id, c.nof_prb, 2, c.sf) for g in grids]
    return csi(np.stack([e[0] for e in est]), mean_noise([e[1] for e in est]), c.nof_prb)
