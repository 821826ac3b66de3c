"""CPU: properties of the PUCCH reference (tests/pucch_ref.py) that hold whoever transcribed the formulas --
resources sharing a PRB are orthogonal per slot (data and DMRS symbols separately), energy sits only in the 12
subcarriers of n_prb[slot], slot 1 sits at the mirrored PRB, every occupied RE has unit modulus, a shortened
subframe's last symbol is empty, and the reference receiver returns the transmitted HARQ-ACK and CQI bits."""
import numpy as np
import pytest

import pucch_ref as R

MIXED_NCS = {1: 3, 2: 4, 3: 3}      # a valid nCS-AN > 0 per deltaPUCCH-Shift


@pytest.mark.parametrize("shortened", [0, 1])
@pytest.mark.parametrize("delta,N_cs", [(d, n) for d in (1, 2, 3) for n in (0, MIXED_NCS[d])])
def test_format1_resources_on_one_prb_are_orthogonal(delta, N_cs, shortened):
    base = dict(cell_id=37, nof_prb=6, sf_idx=3, delta=delta, N_cs=N_cs, n_rb_2=1, gh=1, shortened=shortened)
    T, per = 3 * N_cs // delta, 36 // delta
    n_all = np.arange(T + 2 * per)               # the mixed RB (if any) and the first two format-1 RBs
    m = R.resource(fmt=R.F1A, n_pucch=n_all, **base)["m"]
    pairs = 0
    for mm in np.unique(m):
        ns = n_all[m == mm]
        vec = []
        for i, n in enumerate(ns):
            fmt = (R.F1, R.F1A, R.F1B)[i % 3]
            cfg = dict(base, fmt=fmt, n_pucch=int(n))
            vec.append(R.slot_vectors(R.grid(cfg, ack=i % 4), cfg))
        for s in range(2):
            for part in range(2):
                V = np.stack([v[s][part] for v in vec])
                G = np.abs(V @ V.conj().T)
                energy = np.diag(G).copy()
                assert np.all(energy > 0)
                np.fill_diagonal(G, 0)
                assert G.max() < 1e-5 * energy.min(), (mm, s, part, G.max())
        pairs += len(ns) * (len(ns) - 1) // 2
    assert pairs >= 2 * (per * (per - 1) // 2)


CASES = [dict(fmt=R.F1, n_pucch=7), dict(fmt=R.F1A, n_pucch=0, delta=2, N_cs=2), dict(fmt=R.F1A, n_pucch=40, shortened=1),
         dict(fmt=R.F1B, n_pucch=13, delta=3, N_cs=3, n_rb_2=1, shortened=1), dict(fmt=R.F1B, n_pucch=2, delta=1, N_cs=4),
         dict(fmt=R.F2, n_pucch=5, n_rb_2=1, cqi_len=4), dict(fmt=R.F2A, n_pucch=14, n_rb_2=2, cqi_len=11),
         dict(fmt=R.F2B, n_pucch=12, n_rb_2=1, N_cs=3, cqi_len=1), dict(fmt=R.F2B, n_pucch=30, n_rb_2=3, cqi_len=7, nof_prb=25)]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_grid_shape_and_receiver_round_trip(i):
    cfg = dict(dict(cell_id=101 + i, nof_prb=6, sf_idx=i % 10, rnti=0x1230 + i, gh=i % 2), **CASES[i])
    rng = np.random.default_rng(i)
    nprb = cfg["nof_prb"]
    for ack in range(4):
        cqi = rng.integers(0, 2, cfg.get("cqi_len", 0)).tolist()
        g = R.grid(cfg, ack, cqi)
        res = R.resource(**cfg)
        p0, p1 = int(res["n_prb"][0, 0]), int(res["n_prb"][0, 1])
        assert p1 == nprb - 1 - p0
        mask = np.zeros(g.shape, bool)
        mask[:7, 12 * p0:12 * p0 + 12] = True
        mask[7:, 12 * p1:12 * p1 + 12] = True
        if cfg.get("shortened"):
            assert np.all(g[13] == 0)
            mask[13] = False
        assert np.all(g[~mask] == 0)
        assert np.max(np.abs(np.abs(g[mask]) - 1)) < 1e-6
        back = R.demod(R.grid_to_iq(g, nprb), nprb)
        assert np.max(np.abs(back - g)) < 1e-4
        got_ack, got_cqi = R.receive(back, cfg)
        want_ack = {R.F1: 0, R.F1A: ack & 1, R.F1B: ack, R.F2: 0, R.F2A: ack & 1, R.F2B: ack}[cfg["fmt"]]
        assert got_ack == want_ack and got_cqi == cqi


def test_rejected_configurations_have_no_grid():
    assert R.grid(dict(fmt=R.F1A, delta=4)) is None
    assert R.grid(dict(fmt=R.F1A, delta=2, N_cs=3)) is None
    assert R.grid(dict(fmt=R.F2, cqi_len=12)) is None
    assert R.grid(dict(fmt=R.F2, cqi_len=4, shortened=1)) is None
    assert R.grid(dict(fmt=R.F1A, n_pucch=36 * 6)) is None and R.grid(dict(fmt=R.F1A, n_pucch=36 * 6 - 1)) is not None
