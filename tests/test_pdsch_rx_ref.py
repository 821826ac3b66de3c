"""CPU: two-antenna receive diversity.  The float64 reference of the combining rule (tests/pdsch_rx_ref.py) against
pdsch_ref and against the transmitted symbols, the kernels' combining arithmetic (demap_body.h through the host
emulation's emu_pdsch_llr_rx) against that reference, the diversity scenario the GPU test runs, and the workspace
size of a two-antenna batch."""
import functools

import numpy as np
import pytest

import pdsch_ref as R
import pdsch_ref_util as U
import pdsch_rx_ref as X
from helpers import rel_err
from srsue_amd import abi

TOL = 1e-4          # the project's float tolerance (BASELINE.json north_star) through helpers.rel_err


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


@functools.lru_cache(None)
def demap_cfgs():
    from test_gpu_pdsch_ref import demap_cfgs as cfgs
    return tuple(cfgs())


# ------------------------------------------------------------------------------------------------ 1, 2: the reference
@pytest.mark.parametrize("ports", [1, 2], ids=["tm1", "tm2"])
def test_one_antenna_is_pdsch_ref(ports):
    """equalize_rx with one antenna is pdsch_ref.equalize, value for value"""
    c = R.Cfg(cell_id=9, nof_prb=15, nof_ports=ports, sf=2, cfi=2, tbs=104, Qm=4)
    H = U.channel(c, 3)
    g = U.rx_grid(U.pdsch_symbol_grid(c, 3), H, 20.0, 3)
    for noise in (0.01, 0.0):
        assert np.array_equal(X.equalize_rx([g], [H], c.re_mask(), c.tm, noise), R.equalize(g, H, c.re_mask(), c.tm, noise))
    assert np.array_equal(X.pdsch_llr_rx(c, [g], [H]), R.pdsch_llr(c, g, H))


@pytest.mark.parametrize("Qm", [2, 4, 6])
@pytest.mark.parametrize("ports", [1, 2], ids=["tm1", "tm2"])
def test_noiseless_two_antennas_recover_symbols(ports, Qm):
    """two independent exactly known channels, no noise, no regulariser: the combined symbols are the transmitted ones.
    TM1 through U.channel's three taps.  The SFBC equaliser (C6) is exact only where both REs of a pair see the same
    channel -- with the three taps it is off by 0.15 for one antenna as for two -- so TM2 takes U.channel with one tap
    (per antenna and port a random phase and the phase ramp over the symbols, flat over the subcarriers)."""
    c = R.Cfg(cell_id=5 + Qm, nof_prb=6, nof_ports=ports, sf=4, cfi=1, tbs=104, Qm=Qm)
    mask = c.re_mask()
    rng = np.random.default_rng(0x5B0 + Qm)            # U.pdsch_symbol_grid's draw, so the symbols are known here
    sym = R.modulate(rng.integers(0, 2, int(mask.sum()) * c.Qm), c.Qm)
    grids = U.pdsch_symbol_grid(c, Qm)
    Hs = [U.channel(c, 40 + a, **(dict(taps=(1.0, 0.0, 0.0)) if c.tm == 2 else {})) for a in range(2)]
    x = X.equalize_rx([U.rx_grid(grids, H) for H in Hs], Hs, mask, c.tm, noise=0.0)
    err = float(np.max(np.abs(x - sym)))
    print(f"noiseless tm{c.tm} Qm {Qm}: max |x - sent| {err:.3e}")
    assert err < 1e-9


# ------------------------------------------------------------------------------------------------ 3: the kernel arithmetic
def emu_llr(c, g32s, c32s, noise=0.01):
    cfg = U.to_abi(c)
    out = np.zeros(abi.pdsch_G(cfg), np.float32)
    g = np.ascontiguousarray(np.concatenate(g32s), np.float32)
    h = np.ascontiguousarray(np.concatenate(c32s), np.float32)
    n = abi.emu().emu_pdsch_llr_rx(abi.C.byref(cfg), len(g32s), g.ctypes.data, h.ctypes.data, noise, out.ctypes.data)
    assert n == len(out), n
    return out


@pytest.mark.parametrize("n_rx", [1, 2])
def test_emulated_kernel_llrs_match_reference(n_rx):
    """demap_body.h's demap_llr (equalisation with antenna combining, demapper, descrambling), compiled for the host,
    == pdsch_llr_rx at 1e-4 on the demap_cfgs() set; with one antenna also == pdsch_ref.pdsch_llr"""
    cfgs = demap_cfgs()
    worst = 0.0
    for i, (c, (g32s, c32s)) in enumerate(zip(cfgs, X.demap_rx_inputs(cfgs))):
        g32s, c32s = g32s[:n_rx], c32s[:n_rx]
        got = emu_llr(c, g32s, c32s)
        want = X.pdsch_llr_rx(c, X.as_grids(c, g32s), X.as_ces(c, c32s))
        e = rel_err(got, want)
        worst = max(worst, e)
        assert e < TOL, (i, c.nof_prb, c.nof_ports, c.sf, c.cfi, c.Qm, e)
        if n_rx == 1:
            assert rel_err(got, R.pdsch_llr(c, X.as_grids(c, g32s)[0], X.as_ces(c, c32s)[0])) < TOL, i
    print(f"emulated llr n_rx {n_rx}: worst rel_err {worst:.3e}")
    assert abi.emu().emu_pdsch_llr_rx(abi.C.byref(U.to_abi(cfgs[0])), 3, None, None, 0.01, None) == -1


# ------------------------------------------------------------------------------------------------ 4: diversity scenario
@pytest.mark.parametrize("seed", X.DIV_SEEDS)
@pytest.mark.parametrize("name", list(X.DIV_CASES))
def test_diversity_scenario_reference(name, seed):
    """Each antenna hears one half of the band at 25 dB: the reference receiver fails the TB CRC on either antenna
    alone and decodes the transport block from the two combined (8 iterations)."""
    cfg, tb, iqs = X.div_samples(name, seed)
    grids = [R.ofdm_rx(iq, cfg.nof_prb) for iq in iqs]
    ces = [R.chest(g, cfg.cell_id, cfg.nof_prb, cfg.nof_ports, cfg.sf)[0] for g in grids]
    for a in range(2):
        ok, _, _ = R.dlsch_decode(cfg, R.pdsch_llr(cfg, grids[a], ces[a]), U.qpp(), n_its=8)
        assert not ok, f"antenna {a} alone decodes"
    ok, pay, _ = R.dlsch_decode(cfg, X.pdsch_llr_rx(cfg, grids, ces), U.qpp(), n_its=8)
    assert ok and np.array_equal(pay, tb)


# ------------------------------------------------------------------------------------------------ 5: workspace size
def test_plan_device_bytes_counts_the_antenna_planes():
    """a second antenna adds one grid, one ce and one metrics plane, each buffer rounded to 256 B as the allocator
    rounds it; three antennas are refused with a message"""
    cfgs = [R.Cfg(nof_prb=n, nof_ports=p, tbs=104, Qm=2) for n in (6, 15, 100) for p in (1, 2)]
    plan = abi.Plan().build([U.to_abi(c) for c in cfgs])
    al = lambda n: max((n + 255) // 256 * 256, 256)
    planes = (sum(R.NSYMB * c.W * 8 for c in cfgs), sum(R.NSYMB * c.W * c.nof_ports * 8 for c in cfgs), len(cfgs) * 5 * 4)
    for kw in (dict(), dict(keep_llr=True, compact_ce=False)):
        one, two = plan.device_bytes(n_rx=1, **kw), plan.device_bytes(n_rx=2, **kw)
        assert one == plan.device_bytes(**kw)
        assert two - one == sum(al(2 * p) - al(p) for p in planes), (one, two)
    with pytest.raises(RuntimeError, match="n_rx must be 1 or 2"):
        plan.device_bytes(n_rx=3)
    plan.close()
