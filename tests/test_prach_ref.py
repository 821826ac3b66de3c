"""CPU: properties of the PRACH reference itself (tests/prach_ref.py), so that parity with it means something: the
root table is a permutation in complement pairs whose groups admit exactly the restricted N_CS they are listed
under, the restricted cyclic shifts and their Doppler images never overlap, a preamble has constant modulus in
frequency, different shifts of one root are orthogonal, and the time signal has the stated power, CP and period."""
import numpy as np
import pytest

import prach_ref as R


def test_root_table_is_a_permutation_in_complement_pairs():
    assert sorted(R.ROOTS) == list(range(1, 839))
    assert all(R.ROOTS[i] + R.ROOTS[i + 1] == R.NZC for i in range(0, 838, 2))


def test_root_groups_admit_exactly_their_restricted_ncs():
    """a root is usable with a restricted N_CS iff N_CS <= d_u <= (839 - N_CS) / 2: the largest such N_CS is the one
    its group is listed under, and the roots of the first and last group admit none"""
    assert len(R.GROUPS) == len(R.GROUP_NCS)
    for (first, last), want in zip(R.GROUPS, R.GROUP_NCS):
        for i in range(first, last + 1):
            d = R.d_u(R.ROOTS[i])
            ok = [n for n in R.NCS_RESTRICTED if n <= d <= (R.NZC - n) / 2]
            assert (max(ok) if ok else None) == want, (i, R.ROOTS[i], d)


def test_restricted_shift_windows_and_their_doppler_images_are_disjoint():
    """for every root and every restricted N_CS: the windows [C_v, C_v + N_CS) and their images shifted by +d_u and
    -d_u (mod 839) are mutually disjoint"""
    most = 0
    for u in range(1, R.NZC):
        for N_cs in R.NCS_RESTRICTED:
            cv = R.shifts(u, N_cs, True)
            if not cv:
                continue
            most = max(most, len(cv))
            d = R.d_u(u)
            used = np.zeros(R.NZC, int)
            for c in cv:
                for off in (0, d, -d):
                    used[(c + off + np.arange(N_cs)) % R.NZC] += 1
            assert used.max() == 1, (u, N_cs)
    assert 0 < most <= 64


def test_unrestricted_shifts():
    assert R.shifts(5, 0, False) == [0]
    assert R.shifts(5, 13, False) == [13 * v for v in range(64)]
    assert R.shifts(5, 419, False) == [0, 419]


@pytest.mark.parametrize("u,N_cs", [(129, 13), (1, 119), (838, 22), (419, 46)])
def test_constant_modulus_and_orthogonal_shifts(u, N_cs):
    cv = R.shifts(u, N_cs, False)
    X = [R.freq(u, c) for c in cv[:4]]
    for x in X:
        assert np.allclose(np.abs(x), 1.0, atol=1e-9)
    # the cyclic shift is a phase ramp in frequency
    k = np.arange(R.NZC)
    assert np.allclose(X[1], X[0] * np.exp(2j * np.pi * cv[1] * k / R.NZC), atol=1e-9)
    for a in range(len(X)):
        for b in range(a + 1, len(X)):
            assert abs(np.vdot(R.zc(u, cv[a]), R.zc(u, cv[b]))) < 1e-8 * R.NZC


@pytest.mark.parametrize("nof_prb,config_idx,freq_offset", [(6, 0, 0), (15, 16, 4), (25, 32, 19), (100, 48, 94)])
def test_time_signal_power_cp_and_period(nof_prb, config_idx, freq_offset):
    cfg = dict(nof_prb=nof_prb, config_idx=config_idx, root_seq_idx=22, zero_corr_zone=12, high_speed=0,
               freq_offset=freq_offset, preamble_idx=5)
    r = R.resource(**cfg)
    s = R.iq(cfg)
    assert len(s) == r["N_cp"] + r["N_seq"]
    seq = s[r["N_cp"]:r["N_cp"] + r["N_ifft"]]
    assert np.isclose(np.mean(np.abs(seq) ** 2), R.NZC / r["N_ifft"], rtol=1e-9)
    assert np.allclose(s[:r["N_cp"]], seq[-r["N_cp"]:], atol=1e-12)
    if r["format"] >= 2:
        assert np.allclose(s[r["N_cp"] + r["N_ifft"]:], seq, atol=1e-12)
    # the bins outside the 839 of the preamble are empty
    G = np.fft.fft(seq)
    used = (r["first_bin"] + np.arange(R.NZC)) % r["N_ifft"]
    G[used] = 0
    assert np.max(np.abs(G)) < 1e-8


def test_detector_on_the_reference():
    for hs, zczc, idx, delay in [(0, 12, 0, 0), (0, 12, 63, 5), (0, 0, 40, 3), (1, 4, 9, 2), (1, 12, 33, 4)]:
        cfg = dict(nof_prb=6, config_idx=0, root_seq_idx=300, zero_corr_zone=zczc, high_speed=hs, freq_offset=0,
                   preamble_idx=idx)
        s = R.iq(cfg)
        rx = np.concatenate([np.zeros(delay), s])[:len(s)]
        assert R.detect(rx, cfg) == (idx, delay)


def test_send_tti_rows():
    assert [t for t in range(20) if R.send_tti(0, t)] == [1]
    assert [t for t in range(20) if R.send_tti(12, t)] == [0, 2, 4, 6, 8, 10, 12, 14, 16, 18]
    assert [t for t in range(20) if R.send_tti(63, t)] == [9]
    assert [t for t in range(20) if R.send_tti(6, t, 6)] == [6, 16]
    assert not any(R.send_tti(c, t) for c in R.NA_CONFIGS for t in range(20))
