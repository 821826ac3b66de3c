"""CPU: the CSI reference (tests/csi_ref.py) against itself and known channels, mi_csi_subbands, the host emulation of
csi_kernel (emu_csi) against the reference, and the PUCCH report packer.  No GPU.

Measured here (emu_csi against the reference, the 19 cases of csi_ref.CASES): worst capacity rel_err 2.0e-6 (TOL 1e-4);
CQI cells inside the 0.01 dB guard 7 of 1189 (0.6 %, limit 5 %); smallest decision margin 2.0e-3 (limit 1e-3)."""
import numpy as np
import pytest

import csi_ref as X
import pdsch_sm_ref as S
from srsue_amd import abi


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    pass


def random_H(seed, shape=(50,)):
    rng = np.random.default_rng(0xC51 + seed)
    return (rng.standard_normal(shape + (2, 2)) + 1j * rng.standard_normal(shape + (2, 2))) / np.sqrt(2)


# ------------------------------------------------------------------------------------------------ reference identities
@pytest.mark.parametrize("n", [1.0, 0.1, 1e-3])
def test_closed_form_equals_matrix_inverse(n):
    H = random_H(1)
    for pmi in (1, 2):
        a, b = X.sinr_rank2(H, S.CODEBOOK_2L[pmi], n), X.sinr_rank2_closed(H, S.CODEBOOK_2L[pmi], n)
        assert np.max(np.abs(a - b) / (1 + np.abs(a))) < 1e-9


def test_cdd_identity():
    """The TM3 precoder at an odd RE is codebook index 1 with its layers swapped, so under the alternation the two
    layers' capacities sum to index 1's, whatever the channel: cap[CDD] = (cap[R2][0] + cap[R2][1]) / 2."""
    H = random_H(2)
    even, odd = np.zeros(50, int), np.ones(50, int)
    g1 = X.sinr_rank2(H, S.CODEBOOK_2L[1], 0.05)
    assert np.allclose(X.sinr_rank2(H, S.precoder(3, 0, even), 0.05), g1, rtol=1e-10)
    assert np.allclose(X.sinr_rank2(H, S.precoder(3, 0, odd), 0.05), g1[:, ::-1], rtol=1e-10)
    for name in ("sel_6prb_14dB", "sel_15prb_30dB", "rank_deficient_15prb"):
        r = X.case(name)[5]
        for b in range(1 + r["n_sb"]):
            want = r["cap"][b, X.H_R2].sum() / 2
            assert abs(r["cap"][b, X.H_CDD, 0] - want) < 1e-12 and abs(r["cap"][b, X.H_CDD, 1] - want) < 1e-12
        assert abs(r["cdd_layers"].sum() - r["cap"][0, X.H_R2].sum()) < 1e-12


# ------------------------------------------------------------------------------------------------ known channels
@pytest.mark.parametrize("snr_db", [-5.0, 10.0, 30.0])
@pytest.mark.parametrize("i", range(4))
def test_aligned_channel_selects_its_precoder(i, snr_db):
    """h_a1 = q* h_a0: rank-1 index i (q = 1, -1, j, -j) wins and one layer is reported at any SNR"""
    q = (1, -1, 1j, -1j)[i]
    h0 = X.selective(6, 1, 2, 50 + i)[:, 0]                      # [antenna][14][W]
    ces = np.stack([h0, np.conj(q) * h0], 1)
    r = X.csi(ces, 10 ** (-snr_db / 10), 6)
    assert r["pmi_r1"] == i and r["ri_cl"] == 1
    got = abi.emu_csi(6, 2, 2, X.as_f32(ces)[0], 10 ** (-snr_db / 10))
    assert got.pmi_r1 == i and got.ri_cl == 1


def test_unitary_channel_reports_two_layers():
    W = 72
    ces = np.zeros((2, 2, 14, W), np.complex128)
    ces[0, 0], ces[1, 1] = 1.0, 1.0                               # H = I at every point
    ces[0, 0] *= np.exp(0.3j)
    r = X.csi(ces, 1e-3, 6)
    assert r["ri_cl"] == 2 and r["ri_ol"] == 2
    got = abi.emu_csi(6, 2, 2, X.as_f32(ces)[0], 1e-3)
    assert got.ri_cl == 2 and got.ri_ol == 2
    # each layer sees |c|^2 / (2 n) = 500
    assert abs(r["cap"][0, X.H_R2, 0] - np.log2(501)) < 1e-9 and abs(got.cap_array()[0, X.H_CDD, 1] - np.log2(501)) < 1e-4


# ------------------------------------------------------------------------------------------------ subbands
@pytest.mark.parametrize("nof_prb, n_sb, last", [(6, 0, None), (15, 4, 3), (25, 7, 1), (50, 9, 2), (75, 10, 3),
                                                 (100, 13, 4)])
def test_subbands(nof_prb, n_sb, last):
    k, n = abi.csi_subbands(nof_prb)
    assert n == n_sb and (k, n) == X.subbands(nof_prb)
    if n_sb:
        assert nof_prb - (n - 1) * k == last and 0 < last <= k
    else:
        assert k == 0


def test_subbands_bounds():
    assert abi.csi_subbands(7) == (0, 0) and abi.csi_subbands(8) == (4, 2) and abi.csi_subbands(110) == (8, 14)
    assert abi.csi_subbands(26) == (4, 7) and abi.csi_subbands(27) == (6, 5) and abi.csi_subbands(64) == (8, 8)
    for bad in (0, 5, 111):
        with pytest.raises(ValueError):
            abi.csi_subbands(bad)


# ------------------------------------------------------------------------------------------------ emulation
def test_case_margins():
    """every decision of every case is won by at least MARGIN (relative): a capacity error of TOL cannot flip it"""
    lowest = min((m, name, k) for name, *_ in X.CASES for k, m in X.case(name)[5]["margins"].items())
    print(f"smallest decision margin {lowest[0]:.2e} ({lowest[1]}, {lowest[2]})")
    for name, *_ in X.CASES:
        for k, m in X.case(name)[5]["margins"].items():
            assert m >= X.MARGIN, (name, k, m)


def test_gpu_case_margins():
    """the same for the inputs of tests/test_gpu_csi.py: the uploaded channels, and the IQ cases through the reference
    front end"""
    recs = [(f"upload{n}_{j}", X.upload_case(n, j)[2]) for n in X.UPLOAD for j in range(len(X.UPLOAD[n]))] + \
           [(f"iq_{j}", X.iq_case_reference_front(j)) for j in range(len(X.IQ_CASES))]
    for name, r in recs:
        for k, m in r["margins"].items():
            assert m >= X.MARGIN, (name, k, m)


def test_emu_against_reference():
    worst, out, total = 0.0, 0, 0
    for name, *_ in X.CASES:
        prb, ports, n_rx, f, noise, want = X.case(name)
        got = abi.emu_csi(prb, ports, n_rx, f, noise)
        e, o, t = X.compare(got, want, name)
        assert abs(got.noise - noise) <= 1e-7 * noise
        worst, out, total = max(worst, e), out + o, total + t
    print(f"emu_csi: worst cap rel_err {worst:.2e}; CQI cells inside the guard {out} of {total}")
    assert out <= X.CQI_GUARD_SHARE * total


def test_emu_expected_masks():
    assert X.case("one_port_two_rx_25prb")[5]["valid_mask"] == 0x01
    assert X.case("two_ports_one_rx_15prb")[5]["valid_mask"] == 0x1F
    assert X.case("sel_100prb_30dB")[5]["valid_mask"] == 0xFF and X.case("sel_100prb_30dB")[5]["n_sb"] == 13
    r = X.case("two_ports_one_rx_15prb")[5]
    assert (r["ri_cl"], r["ri_ol"], r["cb_r2"]) == (1, 1, 0)


def test_emu_compact_layout():
    """the four pilot rows alone ([port][4][W]) give the record of the full layout's rows 0, 4, 7, 11"""
    prb, ports, n_rx, f, noise, want = X.case("sel_15prb_14dB")
    full = np.asarray(f).reshape(n_rx, ports, 14, 12 * prb, 2)
    comp = np.ascontiguousarray(full[:, :, list(X.PILOT_ROWS)])
    got = abi.emu_csi(prb, ports, n_rx, comp.view(np.complex64).reshape(n_rx, ports, 4, 12 * prb), noise, compact=True)
    X.compare(got, want, "compact")
    ref = X.csi(comp[..., 0].astype(np.float64) + 1j * comp[..., 1], noise, prb, compact=True)
    assert np.array_equal(ref["cap"], want["cap"])


def test_emu_noise_floor_and_bad_arguments():
    prb, ports, n_rx, f, _, _ = X.case("one_port_one_rx_6prb")
    assert abi.emu_csi(prb, ports, n_rx, f, 0.0).noise == np.float32(1e-9)
    for bad in ((5, 1, 1), (6, 3, 1), (6, 1, 3)):
        with pytest.raises(ValueError):
            abi.emu_csi(bad[0], bad[1], bad[2], np.zeros(bad[2] * bad[1] * 14 * 12 * bad[0], np.complex64), 0.1)


# ------------------------------------------------------------------------------------------------ packer
def record(**kw):
    r = abi.CsiResult()
    r.valid_mask, r.ri_cl, r.ri_ol, r.cb_r2 = 0xFF, 1, 1, 1
    for k, v in kw.items():
        if k == "cqi":
            for (h, layer), c in v.items():
                r.cqi[0][h][layer] = c
        else:
            setattr(r, k, v)
    return r


def bits_of(v, w):
    return [(v >> (w - 1 - i)) & 1 for i in range(w)]


def test_pack_wideband_reports():
    r = record(cqi={(X.H_BASE, 0): 11, (X.H_CDD, 0): 6}, ri_ol=2)
    for tm in (1, 2):
        b, ri = abi.csi_pack_pucch(tm, r)
        assert list(b) == [1, 0, 1, 1] and ri == 1
    b, ri = abi.csi_pack_pucch(3, r)
    assert list(b) == [0, 1, 1, 0] and ri == 2
    r.ri_ol = 1
    b, ri = abi.csi_pack_pucch(3, r)
    assert list(b) == [1, 0, 1, 1] and ri == 1


@pytest.mark.parametrize("pmi", range(4))
def test_pack_tm4_rank1(pmi):
    r = record(pmi_r1=pmi, cqi={(X.H_R1 + pmi, 0): 9, (X.H_R1 + (pmi + 1) % 4, 0): 3})
    b, ri = abi.csi_pack_pucch(4, r)
    assert list(b) == bits_of(9, 4) + bits_of(pmi, 2) and ri == 1 and len(b) == 6


@pytest.mark.parametrize("offset, level", [(0, 0), (1, 1), (2, 2), (3, 3), (5, 3), (-4, 4), (-7, 4), (-3, 5), (-2, 6),
                                           (-1, 7)])
@pytest.mark.parametrize("cb", [1, 2])
def test_pack_tm4_rank2_every_differential_row(cb, offset, level):
    """36.213 Table 7.2-2: offset = CQI of codeword 0 - CQI of codeword 1"""
    c0 = 8
    r = record(ri_cl=2, cb_r2=cb, cqi={(X.H_R2 + cb - 1, 0): c0, (X.H_R2 + cb - 1, 1): c0 - offset,
                                       (X.H_R2 + 2 - cb, 0): 1, (X.H_R2 + 2 - cb, 1): 15})
    b, ri = abi.csi_pack_pucch(4, r)
    assert list(b) == bits_of(c0, 4) + bits_of(level, 3) + [cb - 1] and ri == 2 and len(b) == 8


def test_pack_fits_the_pucch_word_and_refuses_what_is_missing():
    r = record(ri_cl=2, cb_r2=2, cqi={(X.H_R2 + 1, 0): 15, (X.H_R2 + 1, 1): 15})
    b, _ = abi.csi_pack_pucch(4, r)
    assert len(b) <= 11 and abi.pucch_uci(0, b) >> 8 == sum(int(v) << i for i, v in enumerate(b))
    one_port = record(valid_mask=1)
    assert len(abi.csi_pack_pucch(1, one_port)[0]) == 4
    for tm in (0, 5):
        with pytest.raises(ValueError):
            abi.csi_pack_pucch(tm, r)
    with pytest.raises(ValueError):
        abi.csi_pack_pucch(4, one_port)
    with pytest.raises(ValueError):
        abi.csi_pack_pucch(3, record(valid_mask=0x1F, ri_ol=2))
