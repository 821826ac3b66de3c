"""GPU: CSI feedback (mi_dl_csi_*: CQI / PMI / RI from the channel estimates) against tests/csi_ref.py.

Capacities at the project's 1e-4 through helpers.rel_err; valid_mask, subbands and the zero cells exact; the decisions
equal (every case's winning margins are pinned at >= 1e-3 by test_csi_ref.py); CQI equal outside the 0.01 dB guard, at
most 5 % of a test's cells inside it.

(a) uploaded estimates  (b) from IQ  (c) compact estimates  (d) stream ordering and reproducibility  (e) API edges.

Measured on an MI355X: worst capacity rel_err (a) 5.0e-7 with two antennas, 1.8e-6 with one, (b) 7.1e-7, (c) 6.3e-7;
CQI cells inside the guard (a) 3 of 426 and 0 of 26, (b) 0 of 33."""
import ctypes as C

import numpy as np
import pytest
import torch

import csi_ref as X
import pdsch_ref as R
import pdsch_ref_util as U
import pdsch_sm_ref as S
from helpers import rel_err
from srsue_amd import abi
from test_gpu_pdsch_ref import TOL, ri, stream
from test_gpu_rx_div import iq_planes, plane_buffer, plane_part
from test_gpu_split import hip_lib

pytestmark = pytest.mark.gpu

S_OFDM, S_CHEST = 1, 2


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert torch.cuda.is_available() and TOL == X.TOL


def check_guard(out, total, what):
    print(f"{what}: CQI cells inside the guard {out} of {total}")
    assert out <= X.CQI_GUARD_SHARE * total


# ------------------------------------------------------------------------------------------------ (a) uploaded estimates
def upload_batch(n_rx):
    """(cfgs, entry -> physical subframe of csi_ref.UPLOAD[n_rx]): 2-port entries of 6, 15, 25 and 100 PRB with a TM3
    pair and a 1-port TM1 entry between them (two antennas); a 1-port and a 2-port entry (one antenna)"""
    cfgs, phys = [], []
    for j, (prb, ports, _, _) in enumerate(X.UPLOAD[n_rx]):
        if n_rx == 2 and j == X.UPLOAD_PAIR:
            cfgs += S.Pair(3, 0, (2, 2), (104, 104), cell_id=20 + j, nof_prb=prb, sf=1, cfi=1).abi()
            phys += [j, j]
        else:
            cfgs.append(U.to_abi(R.Cfg(cell_id=20 + j, nof_prb=prb, nof_ports=ports, sf=j % 10, tbs=104, Qm=2)))
            phys.append(j)
    return cfgs, phys


@pytest.mark.parametrize("n_rx", [2, 1])
def test_uploaded_estimates(n_rx):
    """CSI alone on uploaded estimates with the noise set explicitly.  100 PRB: W = 1200, several steps of a wavefront's
    64 lanes per subband; 25 PRB: a one-PRB last subband; 6 PRB: no subbands; the cw 1 entry of the pair reports its
    partner's record; the 1-port entry only BASE; one antenna: no rank-2 hypotheses."""
    cfgs, phys = upload_batch(n_rx)
    b = abi.Batch(cfgs, n_rx=n_rx)
    cases = [X.upload_case(n_rx, j) for j in phys]
    b.upload(abi.BUF_CE, plane_buffer(b, abi.BUF_CE, [[c[0][a] for c in cases] for a in range(n_rx)]))
    csi = abi.Csi(b)
    assert csi.n == len(cfgs)
    csi.set_noise([c[1] for c in cases])
    csi.run(stream())
    recs = csi.download()
    worst, out, total = 0.0, 0, 0
    for i, (_, noise, want) in enumerate(cases):
        e, o, t = X.compare(recs[i], want, (n_rx, i))
        assert recs[i].noise == np.float32(noise)
        assert bytes(csi.result(i)) == bytes(recs[i])
        worst, out, total = max(worst, e), out + o, total + t
    if n_rx == 2:
        i = phys.index(X.UPLOAD_PAIR)
        assert cfgs[i + 1].cw == 1 and bytes(recs[i + 1]) == bytes(recs[i])
        assert recs[phys.index(4)].valid_mask == 0x01 and recs[-1].n_sb == 13 and recs[0].n_sb == 0
    else:
        assert [r.valid_mask for r in recs] == [0x01, 0x1F]
    print(f"(a) n_rx {n_rx}: worst cap rel_err {worst:.3e}")
    check_guard(out, total, "(a)")
    # the device records are the downloaded ones
    hip = hip_lib()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    dev = (C.c_uint8 * C.sizeof(recs))()
    assert hip.hipMemcpy(dev, csi.device_ptr(), C.sizeof(recs), 2) == 0 and bytes(dev) == bytes(recs)   # device to host
    csi.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (b) from IQ
def iq_batch(cfgs_of, **kw):
    """a two-antenna batch over the IQ cases' samples: cfgs_of(pair) = the entries of one physical subframe"""
    cases = [X.iq_case(j) for j in range(len(X.IQ_CASES))]
    per_case = [cfgs_of(p) for p, _, _ in cases]
    cfgs = [c for cs in per_case for c in cs]
    iqs = [[U.f32c(s[a]) for cs, (_, _, s) in zip(per_case, cases) for _ in cs] for a in range(2)]
    b = abi.Batch(cfgs, n_rx=2, **kw)
    first = np.cumsum([0] + [len(cs) for cs in per_case])[:-1]
    return b, cases, iq_planes(b, iqs), [int(i) for i in first]


def downloaded_reference(b, i, nof_prb, ports, compact=False):
    """the reference record of entry i from the batch's own estimates and chest noise (so the chest's tolerance does
    not enter)"""
    ce, met = b.download(abi.BUF_CE, np.float32), b.download(abi.BUF_METRICS, np.float32).reshape(2, -1, 5)
    rows, W = (4 if compact else 14), 12 * nof_prb
    ces = np.stack([U.c128(plane_part(b, abi.BUF_CE, ce, a, i, 2 * ports * rows * W)).reshape(ports, rows, W)
                    for a in range(2)])
    return X.csi(ces, X.mean_noise(met[:, i]), nof_prb, compact), ces


def test_from_iq():
    """OFDM | CHEST on the spatial-multiplexing reference's samples (6 PRB pairs), then CSI with the chest's noise"""
    b, cases, d_iq, first = iq_batch(lambda p: p.abi())
    b.run_stages(S_OFDM | S_CHEST, d_iq.data_ptr(), stream())
    csi = abi.Csi(b)
    csi.run(stream())
    out = total = 0
    for j, i in enumerate(first):
        want, _ = downloaded_reference(b, i, 6, 2)
        assert min(want["margins"].values()) >= X.MARGIN, (j, want["margins"])
        got = csi.result(i)
        e, o, t = X.compare(got, want, ("iq", j))
        assert abs(got.noise - want["noise"]) <= 1e-6 * want["noise"]
        assert bytes(csi.result(i + 1)) == bytes(got)
        print(f"(b) case {j}: cap rel_err {e:.3e}, noise {got.noise:.4g}, pmi {got.pmi_r1} cb {got.cb_r2} "
              f"ri {got.ri_cl} / {got.ri_ol}")
        out, total = out + o, total + t
    check_guard(out, total, "(b)")
    csi.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (c) compact layout
def test_compact_layout():
    """the same IQ on a MI_DL_FLAG_CE_COMPACT batch of TM2 / TM1 entries (a full run: the estimates are the four pilot
    rows per port): held to the reference on those rows"""
    def entries(p):
        kw = dict(cell_id=p.c.cell_id, nof_prb=6, sf=p.c.sf, cfi=1, tbs=2216, Qm=6)      # no LLR repetition: compact holds
        return [U.to_abi(R.Cfg(nof_ports=2, **kw))] if p.c.cell_id % 2 else [U.to_abi(R.Cfg(nof_ports=1, **kw))]
    b, cases, d_iq, first = iq_batch(entries, compact_ce=True, max_its=1)
    b.run(d_iq.data_ptr(), stream())
    csi = abi.Csi(b)
    csi.run(stream())
    seen = set()
    for j, i in enumerate(first):
        ports = b.cfgs[i].nof_ports
        seen.add(ports)
        want, ces = downloaded_reference(b, i, 6, ports, compact=True)
        # the layout is the compact one: its rows are the reference front end's pilot rows
        pair, _, iqs = cases[j]
        for a in range(2):
            ref = R.chest(R.ofdm_rx(U.c128(U.f32c(iqs[a])), 6), pair.c.cell_id, 6, ports, pair.c.sf)[0]
            assert rel_err(ri(ces[a]), ri(ref[:, list(X.PILOT_ROWS)])) < TOL
        e, _, _ = X.compare(csi.result(i), want, ("compact", j), decisions=ports == 1 or
                            min(want["margins"].values()) >= X.MARGIN)
        print(f"(c) case {j} ({ports} ports): cap rel_err {e:.3e}")
    assert seen == {1, 2}
    csi.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (d) ordering
def test_stream_order_and_reproducibility():
    """front end and CSI on a non-default stream with no synchronisation between or after them: result() is the
    reference's, and a second run gives the same bytes"""
    b, cases, d_iq, first = iq_batch(lambda p: p.abi())
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    csi = abi.Csi(b)
    b.run_stages(S_OFDM | S_CHEST, d_iq.data_ptr(), st.cuda_stream)
    csi.run(st.cuda_stream)
    one = bytes(csi.download())
    got = csi.result(first[0])
    csi.run(st.cuda_stream)
    two = bytes(csi.download())
    assert one == two
    st.synchronize()
    want, _ = downloaded_reference(b, first[0], 6, 2)
    X.compare(got, want, "ordering")
    csi.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (e) API edges
def test_api_edges():
    L = abi.lib()
    assert not L.mi_dl_csi_create(None) and "null" in abi.last_error()
    assert L.mi_dl_csi_run(None, None) == -1 and L.mi_dl_csi_n(None) == 0 and not L.mi_dl_csi_device_ptr(None)
    cfgs, _ = upload_batch(1)
    b = abi.Batch(cfgs)
    csi = abi.Csi(b)
    with pytest.raises(RuntimeError, match="CHEST"):
        csi.run(stream())                                            # nothing has written the estimates yet
    r = abi.CsiResult()
    assert L.mi_dl_csi_result(csi.h, len(cfgs), C.byref(r)) == -1 and L.mi_dl_csi_result(csi.h, 0, None) == -1
    assert L.mi_dl_csi_download(csi.h, None) == -1 and L.mi_dl_csi_set_noise(None, None) == -1
    with pytest.raises(ValueError):
        csi.set_noise([0.1])                                         # one value per entry
    # uploaded estimates without a noise value still need the chest's metrics
    b.upload(abi.BUF_CE, np.zeros(abi.lib().mi_dl_batch_bytes(b.h, abi.BUF_CE) // 4, np.float32))
    with pytest.raises(RuntimeError, match="CHEST"):
        csi.run(stream())
    csi.set_noise([0.1] * len(cfgs))
    csi.run(stream())
    assert csi.result(0).valid_mask == 1 and not csi.result(1).cap_array().any()   # all-zero estimates: capacity 0
    csi.set_noise(None)
    with pytest.raises(RuntimeError, match="CHEST"):
        csi.run(stream())
    # a re-planned batch: the object describes the old plan
    plan = abi.Plan()
    plan.build(list(reversed(cfgs)))
    b.replan(plan, stream())
    csi.set_noise([0.1] * len(cfgs))
    with pytest.raises(RuntimeError, match="re-planned"):
        csi.run(stream())
    plan.close()
    csi.close()
    b.close()
