"""ctypes bindings of the C ABI in include/mi_dl.h and include/srslte/srslte.h.

The product is the C-ABI shared library srsue_amd/libsrsue_amd.so (gfx950 kernels + host C++);
this module only binds it.  Loading fails loudly if the library has not been built -- there is no
CPU fallback for the receive path.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRSUE_AMD_LIB") or os.path.join(PKG_DIR, "libsrsue_amd.so")
EMU_PATH = os.path.join(PKG_DIR, "libsrsue_amd_emu.so")

MAX_PRB = 110
STAGES = ("ofdm", "chest", "demap", "rm", "tdec", "tb")
BUF_GRID, BUF_CE, BUF_LLR, BUF_PAYLOAD, BUF_TB_CRC, BUF_TB_ITS, BUF_METRICS, BUF_CB_ITS, BUF_CB_CRC, BUF_SB = range(10)
FLAG_PROFILE = 1
FLAG_TDEC_I16 = 2   # int16 ("SSE") turbo arithmetic (the default), see include/mi_dl.h
FLAG_TDEC_GEN = 4   # float srsLTE-gen turbo arithmetic
FLAG_IQ_SC16 = 8    # IQ input as UHD sc16 (int16 I/Q, fc32 = sc16 / 32768)
FLAG_TDEC_WIN = 16  # int16 turbo: force the latency form (one workgroup per code block)
FLAG_TDEC_LANE = 32  # int16 turbo: force one code block per lane of 64-lane wavefronts
FLAG_TDEC_X = 128  # lane-per-code-block decoder, crossed schedule (two wavefronts per group)
FLAG_TDEC_XR = 256  # crossed kernel, recompute form (5 waves per SIMD)
FLAG_TDEC_P2 = 512   # two code blocks per lane (packed int16), crossed
FLAG_CE_COMPACT = 1024  # compact channel estimates (4 pilot rows per port), interpolated in the fused demap
FLAG_TDEC_SEG = 2048  # packed turbo waterfall: late rounds as exact 8-step segments (one stream faster, see mi_dl.h)
SCHED_FLAGS = {None: 0, "auto": 0, "win": FLAG_TDEC_WIN, "lane": FLAG_TDEC_LANE, "lanex": FLAG_TDEC_LANE | FLAG_TDEC_X,
               "lanexr": FLAG_TDEC_LANE | FLAG_TDEC_X | FLAG_TDEC_XR, "p2": FLAG_TDEC_LANE | FLAG_TDEC_P2}
FLAG_KEEP_LLR = 64  # keep the LLR stream of a full run (else demap is fused into rate de-matching)


class SfCfg(C.Structure):
    """mi_dl_sf_cfg_t (include/mi_dl.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("cell_id", "nof_prb", "nof_ports", "sf_idx", "cfi", "tm", "nl_td",
                                          "rnti", "rv", "tbs", "Qm", "new_tb")] + \
               [("prb_mask", C.c_uint8 * MAX_PRB), ("cw", C.c_uint32), ("pmi", C.c_uint32)]


def sf_cfg(cell_id=1, nof_prb=100, nof_ports=1, sf_idx=1, cfi=1, tm=None, rnti=0x46, rv=0, tbs=75376, Qm=6,
           new_tb=1, prb=None, nl_td=2, cw=0, pmi=0):
    """cw / pmi: spatial multiplexing (tm 3 / 4), where a subframe is two consecutive entries cw = 0, cw = 1."""
    c = SfCfg()
    c.cw, c.pmi = cw, pmi
    c.cell_id, c.nof_prb, c.nof_ports, c.sf_idx, c.cfi = cell_id, nof_prb, nof_ports, sf_idx, cfi
    c.tm = tm if tm is not None else (2 if nof_ports == 2 else 1)
    c.nl_td, c.rnti, c.rv, c.tbs, c.Qm, c.new_tb = nl_td, rnti, rv, tbs, Qm, new_tb
    for p in range(MAX_PRB):
        # 0/1 entries (both slots) or the two-slot encoding of mi_dl_sf_cfg_t (bit s = used in slot s)
        c.prb_mask[p] = (1 if prb is None else int(prb[p])) if p < nof_prb else 0
    return c


def cfg_array(cfgs):
    arr = (SfCfg * len(cfgs))()
    for i, c in enumerate(cfgs):
        arr[i] = c
    return arr


_lib = None
_emu = None


def lib():
    """The product library; raises if it is missing (build with __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        sig = {
            "mi_dl_batch_create": (vp, [vp, u32, u32, u32]),
            "mi_dl_batch_create_rx": (vp, [vp, u32, u32, u32, u32]),
            "mi_dl_batch_n_rx": (u32, [vp]),
            "mi_dl_batch_rx_stride": (sz, [vp, C.c_int]),
            "mi_dl_batch_iq_rx_stride": (sz, [vp]),
            "mi_dl_plan_device_bytes_rx": (sz, [vp, u32, u32, u32]),
            "mi_dl_pipe_create_rx": (vp, [vp, u32, u32, u32, u32]),
            "mi_dl_batch_destroy": (None, [vp]),
            "mi_dl_batch_iq_offset": (sz, [vp, u32]),
            "mi_dl_batch_iq_samples": (sz, [vp]),
            "mi_dl_batch_payload_offset": (sz, [vp, u32]),
            "mi_dl_batch_bytes": (sz, [vp, C.c_int]),
            "mi_dl_batch_offset": (sz, [vp, C.c_int, u32]),
            "mi_dl_batch_run": (C.c_int, [vp, vp, vp]),
            "mi_dl_batch_download": (C.c_int, [vp, C.c_int, vp, sz]),
            "mi_dl_batch_run_stages": (C.c_int, [vp, vp, vp, u32]),
            "mi_dl_batch_run_split": (C.c_int, [vp, vp, vp, vp]),
            "mi_dl_batch_upload": (C.c_int, [vp, C.c_int, vp, sz]),
            "mi_dl_batch_device_ptr": (vp, [vp, C.c_int]),
            "mi_dl_batch_stage_ms": (C.c_int, [vp, vp, vp]),
            "mi_dl_batch_profile_reset": (None, [vp]),
            "mi_dl_batch_algo_bytes": (C.c_double, [vp, C.c_int]),
            "mi_dl_batch_n_codeblocks": (u32, [vp]),
            "mi_dl_batch_turbo_win": (C.c_int, [vp]),
            "mi_dl_batch_turbo_compact": (C.c_int, [vp]),
            "mi_tdec_turbo_win": (C.c_int, [vp]),
            "mi_dl_batch_n_groups": (u32, [vp]),
            "mi_dl_batch_rm_direct_groups": (u32, [vp]),
            "mi_dl_batch_set_tdec_history": (C.c_int, [vp, C.c_int]),
            "mi_dl_batch_reset_history": (None, [vp]),
            "mi_dl_plan_create": (vp, []),
            "mi_dl_plan_destroy": (None, [vp]),
            "mi_dl_plan_build": (C.c_int, [vp, vp, u32]),
            "mi_dl_batch_replan": (C.c_int, [vp, vp, vp]),
            "mi_dl_batch_device_bytes": (sz, [vp]),
            "mi_dl_plan_device_bytes": (sz, [vp, u32, u32]),
            "mi_tx_subframe": (C.c_int, [vp, vp, vp, C.c_float, C.c_uint64, vp]),
            "mi_tx_subframe_sm": (C.c_int, [vp, vp, vp, vp, C.c_float, C.c_uint64, vp]),
            "mi_turbo_encode": (C.c_int, [vp, u32, u32, vp]),
            "mi_tdec_create": (vp, [u32, u32, u32, C.c_int, C.c_int, u32]),
            "mi_tdec_destroy": (None, [vp]),
            "mi_tdec_run": (C.c_int, [vp, vp, vp]),
            "mi_tdec_download": (C.c_int, [vp, vp, vp, vp]),
            "mi_tdec_stage_ms": (C.c_int, [vp, vp, vp]),
            "mi_tdec_profile_reset": (None, [vp]),
            "mi_tdec_algo_bytes": (C.c_double, [vp]),
            "mi_sf_len": (C.c_int, [u32]),
            "mi_pdsch_G": (C.c_int, [vp]),
            "mi_dl_ctrl_create": (vp, [vp, u32]),
            "mi_dl_ctrl_create_flags": (vp, [vp, u32, u32]),
            "mi_dl_ctrl_n_jobs": (u32, [vp]),
            "mi_dci_dl2_size": (C.c_int, [u32, u32, u32]),
            "mi_dci_dl2_pack": (C.c_int, [u32, u32, vp, vp]),
            "mi_dci_dl2_unpack": (C.c_int, [u32, u32, u32, vp, u32, vp]),
            "mi_dci_dl2_to_cfg": (C.c_int, [vp, vp, vp, u32, vp]),
            "mi_dl_ctrl_destroy": (None, [vp]),
            "mi_dl_ctrl_run": (C.c_int, [vp, vp]),
            "mi_dl_ctrl_run_stages": (C.c_int, [vp, u32, vp]),
            "mi_dl_ctrl_result": (C.c_int, [vp, u32, C.c_int, vp, vp, vp, vp, vp, vp]),
            "mi_dl_ctrl_llr_floats": (sz, [vp]),
            "mi_dl_ctrl_llr_offset": (sz, [vp, u32]),
            "mi_dl_ctrl_n_cce": (u32, [vp, u32]),
            "mi_dl_ctrl_llr": (C.c_int, [vp, vp, sz, C.c_int]),
            "mi_dl_ctrl_set_phich": (C.c_int, [vp, vp, vp]),
            "mi_dl_ctrl_phich": (C.c_int, [vp, u32, vp]),
            "mi_pbch_re_indices": (C.c_int, [u32, u32, vp]),
            "mi_pbch_create": (vp, [vp]),
            "mi_pbch_destroy": (None, [vp]),
            "mi_pbch_n_frames": (u32, [vp]),
            "mi_pbch_frame_of": (C.c_int, [vp, u32]),
            "mi_pbch_set_candidates": (C.c_int, [vp, vp, vp, u32]),
            "mi_pbch_n_jobs": (u32, [vp]),
            "mi_pbch_run": (C.c_int, [vp, u32, vp]),
            "mi_pbch_result": (C.c_int, [vp, u32, vp]),
            "mi_pbch_llr_floats": (sz, [vp]),
            "mi_pbch_llr": (C.c_int, [vp, vp, sz, C.c_int]),
            "mi_tx_pbch": (C.c_int, [u32, u32, u32, vp, u32, vp, vp]),
            "mi_cellsearch_create": (vp, []),
            "mi_cellsearch_destroy": (None, [vp]),
            "mi_cellsearch_run": (C.c_int, [vp, vp, vp, u32, C.c_float, vp, vp]),
            "mi_acq_create": (vp, [vp, vp]),
            "mi_acq_destroy": (None, [vp]),
            "mi_acq_search": (C.c_int, [vp, u32, C.c_float, vp, vp]),
            "mi_acq_mib": (C.c_int, [vp, u32, C.c_float, u32, vp]),
            "mi_sync_create": (vp, [u32]),
            "mi_sync_destroy": (None, [vp]),
            "mi_sync_fft_size": (u32, [vp]),
            "mi_sync_pss": (C.c_int, [vp, vp, vp, u32, u32, u32, vp, vp]),
            "mi_sync_sss": (C.c_int, [vp, vp, vp, vp, vp, u32, vp, vp]),
            "mi_sync_correct": (C.c_int, [vp, vp, vp, vp, vp, vp, u32, u32, vp]),
            "mi_tx_sync": (C.c_int, [u32, u32, u32, C.c_float, vp]),
            "mi_dl_pipe_create": (vp, [vp, u32, u32, u32]),
            "mi_dl_pipe_destroy": (None, [vp]),
            "mi_dl_pipe_submit": (C.c_int, [vp, vp]),
            "mi_dl_pipe_wait": (C.c_int, [vp, C.c_int]),
            "mi_dl_pipe_batch": (vp, [vp, C.c_int]),
            "mi_host_alloc": (vp, [sz]),
            "mi_host_free": (None, [vp]),
            "mi_device_count": (C.c_int, []),
            "mi_set_device": (C.c_int, [C.c_int]),
            "mi_last_error": (C.c_char_p, []),
            "mi_stream_create_cu_share": (C.c_int, [u32, u32, vp]),
            "mi_stream_destroy": (C.c_int, [vp]),
            "mi_ul_batch_create": (vp, [vp, u32, u32]),
            "mi_ul_batch_destroy": (None, [vp]),
            "mi_ul_batch_payload_offset": (sz, [vp, u32]),
            "mi_ul_batch_payload_bytes": (sz, [vp]),
            "mi_ul_batch_iq_offset": (sz, [vp, u32]),
            "mi_ul_batch_iq_samples": (sz, [vp]),
            "mi_ul_batch_n_codeblocks": (u32, [vp]),
            "mi_ul_batch_run": (C.c_int, [vp, vp, vp, vp]),
            "mi_ul_batch_symbols": (C.c_int, [vp, u32, vp]),
            "mi_ul_batch_stage_ms": (C.c_int, [vp, vp, vp]),
            "mi_ul_batch_profile_reset": (None, [vp]),
            "mi_ul_batch_algo_bytes": (C.c_double, [vp]),
            "mi_ul_pusch_resource": (C.c_int, [vp, vp]),
            "mi_ul_pusch_n_srs": (C.c_int, [u32, u32, u32, u32, u32, u32, u32, C.c_int, u32]),
            "mi_ul_pusch_power_nsymb": (C.c_float, [vp, C.c_float, C.c_float, u32, u32, u32]),
            "mi_pucch_resource": (C.c_int, [vp, vp]),
            "mi_pucch_resource_n": (u32, [vp, u32, vp]),
            "mi_pucch_select": (C.c_int, [u32, C.c_int, u32, C.c_int, u32, u32, u32, u32, vp]),
            "mi_pucch_batch_create": (vp, [vp, u32, u32]),
            "mi_pucch_batch_destroy": (None, [vp]),
            "mi_pucch_batch_iq_offset": (sz, [vp, u32]),
            "mi_pucch_batch_iq_samples": (sz, [vp]),
            "mi_pucch_batch_run": (C.c_int, [vp, vp, vp, vp]),
            "mi_pucch_batch_resource": (C.c_int, [vp, u32, vp]),
            "mi_prach_resource": (C.c_int, [vp, vp]),
            "mi_prach_resource_n": (u32, [vp, u32, vp]),
            "mi_prach_root": (C.c_int, [u32]),
            "mi_prach_format": (C.c_int, [u32]),
            "mi_prach_send_tti": (C.c_int, [u32, u32, C.c_int]),
            "mi_prach_batch_create": (vp, [vp, u32, u32]),
            "mi_prach_batch_destroy": (None, [vp]),
            "mi_prach_batch_iq_offset": (sz, [vp, u32]),
            "mi_prach_batch_iq_samples": (sz, [vp]),
            "mi_prach_batch_run": (C.c_int, [vp, vp, vp, vp, vp]),
            "mi_prach_batch_resource": (C.c_int, [vp, u32, vp]),
            "mi_srs_resource": (C.c_int, [vp, vp]),
            "mi_srs_resource_n": (u32, [vp, u32, vp]),
            "mi_srs_batch_create": (vp, [vp, u32, u32]),
            "mi_srs_batch_destroy": (None, [vp]),
            "mi_srs_batch_iq_offset": (sz, [vp, u32]),
            "mi_srs_batch_iq_samples": (sz, [vp]),
            "mi_srs_batch_run": (C.c_int, [vp, vp, vp, vp, vp]),
            "mi_srs_batch_resource": (C.c_int, [vp, u32, vp]),
            "mi_ul_pusch_power": (C.c_float, [vp, C.c_float, C.c_float, u32, u32]),
            "mi_ul_pucch_power": (C.c_float, [vp, C.c_float, u32, u32, u32]),
            "mi_ul_srs_power": (C.c_float, [vp, C.c_float, u32]),
            "mi_dl_csi_create": (vp, [vp]),
            "mi_dl_csi_destroy": (None, [vp]),
            "mi_dl_csi_n": (u32, [vp]),
            "mi_dl_csi_set_noise": (C.c_int, [vp, vp]),
            "mi_dl_csi_run": (C.c_int, [vp, vp]),
            "mi_dl_csi_result": (C.c_int, [vp, u32, vp]),
            "mi_dl_csi_download": (C.c_int, [vp, vp]),
            "mi_dl_csi_device_ptr": (vp, [vp]),
            "mi_csi_subbands": (C.c_int, [u32, vp, vp]),
            "mi_csi_pack_pucch": (C.c_int, [u32, vp, vp, vp]),
        }
        # the receive-diversity, CSI and format 2 / 2A entry points are absent from a library built before them, which an
        # A/B run selects with SRSUE_AMD_LIB (tools/ab_libs.sh): such a library binds without them, and calling one raises
        rx_names = {n for n in sig if n.endswith("_rx") or "_rx_" in n or "_csi_" in n or "_dci_dl2_" in n or
                    n in ("mi_dl_batch_n_rx", "mi_tx_subframe_sm", "mi_dl_ctrl_create_flags", "mi_dl_ctrl_n_jobs")}
        for name, (res, args) in sig.items():
            if name in rx_names and "SRSUE_AMD_LIB" in os.environ and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def emu():
    """TEST-ONLY host emulation of the per-lane kernel bodies (never used by the product path)."""
    global _emu
    if _emu is None:
        E = C.CDLL(EMU_PATH)
        E.emu_decode_llr.restype = C.c_int
        E.emu_decode_llr.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
        E.emu_set_tdec_i16.restype = None
        E.emu_set_tdec_i16.argtypes = [C.c_int]
        E.emu_set_tdec_x.restype = None
        E.emu_set_tdec_x.argtypes = [C.c_int]
        E.emu_keep_softbuffer.restype = None
        E.emu_keep_softbuffer.argtypes = [C.c_int]
        E.emu_payload_offset.restype = C.c_size_t
        E.emu_payload_offset.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        E.emu_pdsch_llr_rx.restype = C.c_int
        E.emu_pdsch_llr_rx.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        E.emu_softbuffer.restype = C.c_size_t
        E.emu_softbuffer.argtypes = [C.c_void_p]
        E.emu_plan_info.restype = C.c_int
        E.emu_plan_info.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        E.emu_last_error.restype = C.c_char_p
        E.emu_last_error.argtypes = []
        E.emu_pdsch_llr_sm.restype = C.c_int
        E.emu_pdsch_llr_sm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        E.emu_csi.restype = C.c_int
        E.emu_csi.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_float, C.c_void_p]
        E.emu_pdcch_llr_rx.restype = C.c_int
        E.emu_pdcch_llr_rx.argtypes = [C.c_uint32] * 7 + [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        _emu = E
    return _emu


def last_error():
    return lib().mi_last_error().decode()


def stream_cu_share(first, count):
    """A HIP stream (handle as int) on the CUs whose index mod 8 lies in [first, first + count) (mi_stream_create_cu_share);
    release with stream_destroy."""
    h = C.c_void_p()
    if lib().mi_stream_create_cu_share(first, count, C.byref(h)):
        raise RuntimeError("mi_stream_create_cu_share: " + last_error())
    return h.value


def stream_destroy(h):
    if lib().mi_stream_destroy(C.c_void_p(h)):
        raise RuntimeError("mi_stream_destroy: " + last_error())


def tx_subframe(cfg, tb_bytes, h=None, snr_db=30.0, seed=0xA5A5):
    """Synthetic subframe from the product transmitter (mi_tx_subframe)."""
    n = lib().mi_sf_len(cfg.nof_prb)
    iq = np.zeros(2 * n, np.float32)
    hh = None
    if h is not None:
        hh = np.zeros(4, np.float32)
        for p, v in enumerate(h[:2]):
            hh[2 * p], hh[2 * p + 1] = v.real, v.imag
    tb = np.ascontiguousarray(tb_bytes, np.uint8)
    rc = lib().mi_tx_subframe(C.byref(cfg), tb.ctypes.data, None if hh is None else hh.ctypes.data,
                              float(snr_db), seed, iq.ctypes.data)
    if rc:
        raise RuntimeError("mi_tx_subframe failed")
    return iq


def tx_subframe_sm(cfg_pair, tb0, tb1, h=None, snr_db=30.0, seed=0xA5A5):
    """One receive antenna's samples of a spatially multiplexed subframe (mi_tx_subframe_sm): cfg_pair = its cw 0 and
    cw 1 entries, h = that antenna's flat channel per port.  Call once per receive antenna."""
    n = lib().mi_sf_len(cfg_pair[0].nof_prb)
    iq = np.zeros(2 * n, np.float32)
    hh = None
    if h is not None:
        hh = np.zeros(4, np.float32)
        for p, v in enumerate(h[:2]):
            hh[2 * p], hh[2 * p + 1] = v.real, v.imag
    arr = cfg_array(list(cfg_pair))
    t0, t1 = np.ascontiguousarray(tb0, np.uint8), np.ascontiguousarray(tb1, np.uint8)
    rc = lib().mi_tx_subframe_sm(C.cast(arr, C.c_void_p), t0.ctypes.data, t1.ctypes.data,
                                 None if hh is None else hh.ctypes.data, float(snr_db), seed, iq.ctypes.data)
    if rc:
        raise RuntimeError("mi_tx_subframe_sm failed")
    return iq


class Batch:
    """Owns one mi_dl_batch_t (planned once; run() only enqueues kernels)."""

    def __init__(self, cfgs, max_its=4, profile=False, tdec_i16=True, iq_sc16=False, sched=None, keep_llr=False,
                 compact_ce=False, seg_rounds=False, n_rx=1, rx_entry=False):
        """n_rx: receive antennas (1 or 2); the IQ, grid, ce and metrics buffers then hold n_rx planes (rx_stride).
        One antenna is created through mi_dl_batch_create unless rx_entry asks for mi_dl_batch_create_rx."""
        self.cfgs = list(cfgs)
        self._arr = cfg_array(self.cfgs)
        flags = (FLAG_PROFILE if profile else 0) | (FLAG_TDEC_I16 if tdec_i16 else FLAG_TDEC_GEN) | \
            (FLAG_IQ_SC16 if iq_sc16 else 0) | SCHED_FLAGS[sched] | (FLAG_KEEP_LLR if keep_llr else 0) | \
            (FLAG_CE_COMPACT if compact_ce else 0) | (FLAG_TDEC_SEG if seg_rounds else 0)
        if n_rx == 1 and not rx_entry:
            self.h = lib().mi_dl_batch_create(C.cast(self._arr, C.c_void_p), len(self.cfgs), max_its, flags)
        else:
            self.h = lib().mi_dl_batch_create_rx(C.cast(self._arr, C.c_void_p), len(self.cfgs), n_rx, max_its, flags)
        if not self.h:
            raise RuntimeError("mi_dl_batch_create: " + last_error())

    @classmethod
    def view(cls, handle, cfgs):
        """Non-owning wrapper of a batch owned elsewhere (a pipe slot)."""
        b = cls.__new__(cls)
        b.cfgs, b._arr, b.h, b._owned = list(cfgs), None, handle, False
        return b

    def close(self):
        if self.h and getattr(self, "_owned", True):
            lib().mi_dl_batch_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def iq_samples(self):
        return lib().mi_dl_batch_iq_samples(self.h)

    def iq_offset(self, sf):
        return lib().mi_dl_batch_iq_offset(self.h, sf)

    @property
    def n_rx(self):
        return lib().mi_dl_batch_n_rx(self.h)

    def rx_stride(self, which):
        """elements (the units of offset()) between the antenna planes of buffer `which`"""
        return lib().mi_dl_batch_rx_stride(self.h, which)

    @property
    def iq_rx_stride(self):
        """samples between the antenna planes of the IQ buffer"""
        return lib().mi_dl_batch_iq_rx_stride(self.h)

    def run(self, d_iq_ptr, stream_ptr=None):
        rc = lib().mi_dl_batch_run(self.h, C.c_void_p(d_iq_ptr), C.c_void_p(stream_ptr or 0))
        if rc:
            raise RuntimeError("mi_dl_batch_run: " + last_error())

    def replan(self, plan, stream_ptr=None):
        """Swap plan's built configuration in (mi_dl_batch_replan): table upload enqueued on stream_ptr, the
        stream this batch runs on; plan then holds the previous configuration's data, ready for a rebuild."""
        cfgs = plan.cfgs
        if lib().mi_dl_batch_replan(self.h, plan.h, C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_dl_batch_replan: " + last_error())
        plan.cfgs, self.cfgs = self.cfgs, cfgs

    def run_split(self, d_iq_ptr, front_ptr, back_ptr):
        """mi_dl_batch_run_split: front end on front_ptr, turbo decoder + TB CRC on back_ptr (complete with it)."""
        rc = lib().mi_dl_batch_run_split(self.h, C.c_void_p(d_iq_ptr), C.c_void_p(front_ptr or 0),
                                         C.c_void_p(back_ptr or 0))
        if rc:
            raise RuntimeError("mi_dl_batch_run_split: " + last_error())

    def run_stages(self, mask, d_iq_ptr=None, stream_ptr=None):
        rc = lib().mi_dl_batch_run_stages(self.h, C.c_void_p(d_iq_ptr or 0), C.c_void_p(stream_ptr or 0), mask)
        if rc:
            raise RuntimeError("mi_dl_batch_run_stages: " + last_error())

    def upload(self, which, host_array):
        a = np.ascontiguousarray(host_array)
        if lib().mi_dl_batch_upload(self.h, which, a.ctypes.data, a.nbytes):
            raise RuntimeError("upload: " + last_error())

    def download(self, which, dtype):
        n = lib().mi_dl_batch_bytes(self.h, which)
        out = np.zeros(n // np.dtype(dtype).itemsize, dtype)
        if lib().mi_dl_batch_download(self.h, which, out.ctypes.data, n):
            raise RuntimeError("download: " + last_error())
        return out

    def offset(self, which, sf):
        return lib().mi_dl_batch_offset(self.h, which, sf)

    def stage_ms(self):
        """Per-stage device ms averaged over the profiled runs since profile_reset()."""
        ms = np.zeros(len(STAGES), np.float32)
        n = C.c_uint32(0)
        if lib().mi_dl_batch_stage_ms(self.h, ms.ctypes.data, C.byref(n)):
            raise RuntimeError("stage_ms: " + last_error())
        return dict(zip(STAGES, ms.tolist())), n.value

    def profile_reset(self):
        lib().mi_dl_batch_profile_reset(self.h)

    def algo_bytes(self, stage=-1):
        return lib().mi_dl_batch_algo_bytes(self.h, stage)

    @property
    def n_codeblocks(self):
        return lib().mi_dl_batch_n_codeblocks(self.h)

    @property
    def turbo_win(self):
        """True when the turbo stage runs the latency form (one workgroup per code block)."""
        return lib().mi_dl_batch_turbo_win(self.h) == 1

    @property
    def turbo_sched(self):
        """'win' (latency form), 'lanex' (lane per code block, two wavefronts per group) or 'lane'"""
        return {1: "win", 2: "lanex", 3: "lanexr", 4: "p2"}.get(lib().mi_dl_batch_turbo_win(self.h), "lane")

    @property
    def turbo_compact(self):
        """True when the packed decoder compacts the CRC-failing code blocks after iteration 0 (tdec.hip)."""
        return lib().mi_dl_batch_turbo_compact(self.h) == 1

    @property
    def n_groups(self):
        return lib().mi_dl_batch_n_groups(self.h)

    @property
    def rm_direct_groups(self):
        """groups rate-de-matched in the direct form (rm.hip rm_direct_kernel; MI_RM_DIRECT=0 disables)"""
        return lib().mi_dl_batch_rm_direct_groups(self.h)

    @property
    def device_bytes(self):
        """HBM this batch holds (mi_dl_batch_device_bytes)."""
        return lib().mi_dl_batch_device_bytes(self.h)

    def set_tdec_history(self, mode):
        """Waterfall compaction's schedule source (mi_dl_batch_set_tdec_history): -1 = this batch's history of
        continuation counts (default), 0 = fixed high-SNR schedule, 1 = fixed waterfall schedule (results identical)."""
        if lib().mi_dl_batch_set_tdec_history(self.h, int(mode)):
            raise RuntimeError("set_tdec_history: " + last_error())

    def reset_history(self):
        lib().mi_dl_batch_reset_history(self.h)

    def payload(self, sf, all_payload=None):
        p = all_payload if all_payload is not None else self.download(BUF_PAYLOAD, np.uint8)
        off = lib().mi_dl_batch_payload_offset(self.h, sf)
        return p[off:off + self.cfgs[sf].tbs // 8]


class Plan:
    """Owns one mi_dl_plan_t: host-only planning of a batch (no GPU call; ctypes releases the GIL, so worker
    threads plan while the main thread keeps the GPU busy), swapped into a Batch by Batch.replan()."""

    def __init__(self):
        self.h = lib().mi_dl_plan_create()
        self.cfgs = None

    def build(self, cfgs):
        """cfgs: a list of SfCfg, or a prebuilt cfg_array (no per-call Python conversion)."""
        arr = cfgs if isinstance(cfgs, C.Array) else cfg_array(list(cfgs))
        self.cfgs = arr
        if lib().mi_dl_plan_build(self.h, C.cast(arr, C.c_void_p), len(arr)):
            raise RuntimeError("mi_dl_plan_build: " + last_error())
        return self

    def device_bytes(self, max_its=4, compact_ce=True, keep_llr=False, tdec_i16=True, n_rx=1):
        """HBM a batch of this plan with n_rx receive antennas would allocate for its work buffers and softbuffer
        (mi_dl_plan_device_bytes_rx; host only)."""
        flags = (FLAG_TDEC_I16 if tdec_i16 else FLAG_TDEC_GEN) | (FLAG_CE_COMPACT if compact_ce else 0) | \
            (FLAG_KEEP_LLR if keep_llr else 0)
        n = lib().mi_dl_plan_device_bytes(self.h, max_its, flags) if n_rx == 1 else \
            lib().mi_dl_plan_device_bytes_rx(self.h, max_its, flags, n_rx)
        if not n:
            raise RuntimeError("mi_dl_plan_device_bytes: " + last_error())
        return n

    def close(self):
        if self.h:
            lib().mi_dl_plan_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ctrl:
    """DL control channels over a batch's grid / channel estimates (mi_dl_ctrl_*)."""
    PCFICH, LLR, SEARCH, PHICH = 1, 2, 4, 8
    FLAG_RX_COMBINE, FLAG_TM_FORMATS = 1, 2

    def __init__(self, batch, phich_ng=2, combine=False, tm_formats=False):
        """combine: a two-antenna batch's PCFICH, PDCCH soft bits and PHICH combine both planes (else plane 0 alone);
        tm_formats: the UE-specific space's second DCI size follows the entry's tm (format 2A for tm 3, 2 for tm 4) and
        the cw = 1 entry of a pair reports its partner's results (mi_dl_ctrl_create_flags)."""
        self.batch = batch
        flags = (self.FLAG_RX_COMBINE if combine else 0) | (self.FLAG_TM_FORMATS if tm_formats else 0)
        self.h = lib().mi_dl_ctrl_create_flags(batch.h, phich_ng, flags) if flags else \
            lib().mi_dl_ctrl_create(batch.h, phich_ng)
        if not self.h:
            raise RuntimeError("mi_dl_ctrl_create: " + last_error())

    @property
    def n_jobs(self):
        """(candidate, DCI size) decodes of one run"""
        return lib().mi_dl_ctrl_n_jobs(self.h)

    def set_phich(self, i_lowest, n_dmrs):
        """per-subframe PHICH queries: the UL grant's lowest PRB index and DMRS cyclic shift"""
        a = np.ascontiguousarray(i_lowest, np.uint32)
        b = np.ascontiguousarray(n_dmrs, np.uint32)
        if lib().mi_dl_ctrl_set_phich(self.h, a.ctypes.data, b.ctypes.data):
            raise RuntimeError("mi_dl_ctrl_set_phich: " + last_error())

    def phich(self, sf):
        """(ack, soft HI) of subframe sf after a run with the PHICH stage"""
        s = C.c_float()
        rc = lib().mi_dl_ctrl_phich(self.h, sf, C.byref(s))
        if rc < 0:
            raise RuntimeError("mi_dl_ctrl_phich: " + last_error())
        return rc == 1, s.value

    def run(self, stream_ptr=None, mask=15):
        if lib().mi_dl_ctrl_run_stages(self.h, mask, C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_dl_ctrl_run: " + last_error())

    def result(self, sf, ul=False):
        """(cfi, found DCI or None); DCI = (format, bits, L, ncce)"""
        v = [C.c_uint32() for _ in range(5)]
        bits = np.zeros(64, np.uint8)
        rc = lib().mi_dl_ctrl_result(self.h, sf, int(ul), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]),
                                     bits.ctypes.data, C.byref(v[4]))
        if rc < 0:
            raise RuntimeError("mi_dl_ctrl_result: " + last_error())
        return v[0].value, ((v[1].value, bits[:v[4].value].copy(), v[2].value, v[3].value) if rc == 1 else None)

    def llr(self):
        n = lib().mi_dl_ctrl_llr_floats(self.h)
        out = np.zeros(n, np.float32)
        if lib().mi_dl_ctrl_llr(self.h, out.ctypes.data, n, 0):
            raise RuntimeError("mi_dl_ctrl_llr: " + last_error())
        return out

    def set_llr(self, host):
        a = np.ascontiguousarray(host, np.float32)
        if lib().mi_dl_ctrl_llr(self.h, a.ctypes.data, a.size, 1):
            raise RuntimeError("mi_dl_ctrl_llr: " + last_error())

    def llr_offset(self, sf):
        return lib().mi_dl_ctrl_llr_offset(self.h, sf)

    def n_cce(self, sf):
        return lib().mi_dl_ctrl_n_cce(self.h, sf)

    def close(self):
        if self.h:
            lib().mi_dl_ctrl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DCI_2, DCI_2A = 4, 5


class _Dci2Tb(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("mcs", "ndi", "rv", "enabled")]


class Dci2(C.Structure):
    """mi_dci_dl2_t: an unpacked DCI format 2 / 2A (36.212 5.3.3.1.5 / 5.3.3.1.5A)"""
    _fields_ = [(n, C.c_uint32) for n in ("format", "alloc_type", "type0_alloc", "type1_subset", "type1_shift",
                                          "type1_bitmap", "tpc_pucch", "harq_process", "tb_cw_swap")] + \
               [("tb", _Dci2Tb * 2), ("pinfo", C.c_uint32)]

    def as_tuple(self):
        return tuple(getattr(self, n) for n, _ in self._fields_[:9]) + \
            tuple((t.mcs, t.ndi, t.rv, t.enabled) for t in self.tb) + (self.pinfo,)


def dci2(format=DCI_2, alloc_type=0, type0_alloc=0, type1_subset=0, type1_shift=0, type1_bitmap=0, tpc_pucch=0,
         harq_process=0, tb_cw_swap=0, tb=((0, 0, 0), (0, 0, 0)), pinfo=0):
    """tb: (mcs, ndi, rv) of TB 1 and TB 2; a TB is disabled by mcs = 0, rv = 1"""
    d = Dci2(format, alloc_type, type0_alloc, type1_subset, type1_shift, type1_bitmap, tpc_pucch, harq_process,
             tb_cw_swap)
    for t, (mcs, ndi, rv) in enumerate(tb):
        d.tb[t] = _Dci2Tb(mcs, ndi, rv, int(not (mcs == 0 and rv == 1)))
    d.pinfo = pinfo
    return d


def dci2_size(format, nof_prb, nof_ports=2):
    n = lib().mi_dci_dl2_size(format, nof_prb, nof_ports)
    if n < 0:
        raise ValueError("mi_dci_dl2_size: " + last_error())
    return n


def dci2_pack(nof_prb, d, nof_ports=2):
    """payload bits (one per byte, MSB first) of a Dci2"""
    bits = np.zeros(64, np.uint8)
    n = lib().mi_dci_dl2_pack(nof_prb, nof_ports, C.byref(d), bits.ctypes.data)
    if n < 0:
        raise ValueError("mi_dci_dl2_pack: " + last_error())
    return bits[:n].copy()


def dci2_unpack(format, nof_prb, bits, nof_ports=2):
    b = np.ascontiguousarray(bits, np.uint8)
    d = Dci2()
    if lib().mi_dci_dl2_unpack(format, nof_prb, nof_ports, b.ctypes.data, len(b), C.byref(d)):
        raise ValueError("mi_dci_dl2_unpack: " + last_error())
    return d


def dci2_to_cfgs(d, base, new_tb=(1, 1), reported_cb_r2=0):
    """the one or two batch entries (SfCfg) that decode grant d in the subframe of base (mi_dci_dl2_to_cfg)"""
    out = (SfCfg * 2)()
    nt = np.array(new_tb, np.uint8)
    n = lib().mi_dci_dl2_to_cfg(C.byref(d), C.byref(base), nt.ctypes.data, reported_cb_r2, C.cast(out, C.c_void_p))
    if n < 0:
        raise ValueError("mi_dci_dl2_to_cfg: " + last_error())
    res = []
    for i in range(n):
        c = SfCfg()
        C.memmove(C.byref(c), C.byref(out[i]), C.sizeof(SfCfg))
        res.append(c)
    return res


def emu_pdcch_llr_rx(cell_id, nof_prb, nof_ports, phich_ng, cfi, sf_idx, grids, ces, noise=0.0):
    """TEST-ONLY: the PDCCH soft bits (logical order) of one subframe from the host emulation of the antenna-combining
    pdcch_llr_kernel; grids [n_rx][14][12 nof_prb], ces [n_rx][ports][14][12 nof_prb], complex"""
    g = np.ascontiguousarray(grids, np.complex64)
    h = np.ascontiguousarray(ces, np.complex64)
    n_rx = g.shape[0]
    if g.size != n_rx * 14 * 12 * nof_prb or h.size != g.size * nof_ports:
        raise ValueError("emu_pdcch_llr_rx: arrays do not match the configuration")
    out = np.zeros(8 * 12 * nof_prb, np.float32)   # at most 3 REGs per PRB in each of at most 4 control symbols
    M = emu().emu_pdcch_llr_rx(cell_id, nof_prb, nof_ports, phich_ng, cfi, sf_idx, n_rx, g.ctypes.data, h.ctypes.data,
                               float(noise), out.ctypes.data)
    if M < 0:
        raise ValueError("emu_pdcch_llr_rx: bad configuration")
    return out[:8 * M].copy()


CSI_NHYP, CSI_MAX_SB = 8, 14
CSI_H_BASE, CSI_H_R1, CSI_H_CDD, CSI_H_R2 = 0, 1, 5, 6


class CsiResult(C.Structure):
    """mi_dl_csi_result_t: cap / cqi are [band][hypothesis][layer], band 0 = the whole bandwidth"""
    _fields_ = [(n, C.c_uint32) for n in ("valid_mask", "n_sb", "sb_prb", "pmi_r1", "cb_r2", "ri_cl", "ri_ol")] + \
               [("noise", C.c_float), ("cap", C.c_float * 2 * CSI_NHYP * (1 + CSI_MAX_SB)),
                ("cqi", C.c_uint8 * 2 * CSI_NHYP * (1 + CSI_MAX_SB))]

    def cap_array(self):
        return np.ctypeslib.as_array(self.cap).copy()

    def cqi_array(self):
        return np.ctypeslib.as_array(self.cqi).copy()


def csi_subbands(nof_prb):
    """(subband size in PRB, number of subbands) of 36.213 Table 7.2.1-3 (mi_csi_subbands); (0, 0) = none"""
    k, n = C.c_uint32(), C.c_uint32()
    if lib().mi_csi_subbands(nof_prb, C.byref(k), C.byref(n)):
        raise ValueError("mi_csi_subbands: " + last_error())
    return k.value, n.value


def csi_pack_pucch(tm, res):
    """(bits MSB first, rank) of the PUCCH format 2 CQI / PMI report of a CsiResult (mi_csi_pack_pucch)"""
    bits = np.zeros(11, np.uint8)
    ri = C.c_uint32()
    n = lib().mi_csi_pack_pucch(tm, C.byref(res), bits.ctypes.data, C.byref(ri))
    if n < 0:
        raise ValueError("mi_csi_pack_pucch: " + last_error())
    return bits[:n].copy(), ri.value


def emu_csi(nof_prb, ports, n_rx, ces, noise, compact=False):
    """TEST-ONLY: the CSI record of one subframe from the host emulation of csi_kernel; ces [n_rx][ports][14 or 4]
    [12 nof_prb], complex or interleaved float32"""
    a = np.asarray(ces)
    a = np.ascontiguousarray(a, np.complex64) if np.iscomplexobj(a) else np.ascontiguousarray(a, np.float32).view(np.complex64)
    if a.size != n_rx * ports * (4 if compact else 14) * 12 * nof_prb:
        raise ValueError("emu_csi: estimates do not match the configuration")
    r = CsiResult()
    if emu().emu_csi(nof_prb, ports, n_rx, int(compact), a.ctypes.data, float(noise), C.byref(r)):
        raise ValueError("emu_csi: bad configuration")
    return r


class Csi:
    """CSI feedback (CQI / PMI / RI) over a batch's channel estimates (mi_dl_csi_*); describes the plan the batch
    held when it was created."""

    def __init__(self, batch):
        self.batch = batch
        self.h = lib().mi_dl_csi_create(batch.h)
        if not self.h:
            raise RuntimeError("mi_dl_csi_create: " + last_error())

    @property
    def n(self):
        return lib().mi_dl_csi_n(self.h)

    def set_noise(self, per_sf=None):
        """one noise value per batch entry, or None = the chest metrics (the default)"""
        if per_sf is None:
            rc = lib().mi_dl_csi_set_noise(self.h, None)
        else:
            a = np.ascontiguousarray(per_sf, np.float32)
            if a.size != self.n:
                raise ValueError("set_noise: one value per batch entry")
            rc = lib().mi_dl_csi_set_noise(self.h, a.ctypes.data)
        if rc:
            raise RuntimeError("mi_dl_csi_set_noise: " + last_error())

    def run(self, stream_ptr=None):
        if lib().mi_dl_csi_run(self.h, C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_dl_csi_run: " + last_error())

    def result(self, sf):
        r = CsiResult()
        if lib().mi_dl_csi_result(self.h, sf, C.byref(r)):
            raise RuntimeError("mi_dl_csi_result: " + last_error())
        return r

    def download(self):
        """every entry's record (a ctypes array of CsiResult)"""
        arr = (CsiResult * self.n)()
        if lib().mi_dl_csi_download(self.h, C.cast(arr, C.c_void_p)):
            raise RuntimeError("mi_dl_csi_download: " + last_error())
        return arr

    def device_ptr(self):
        return lib().mi_dl_csi_device_ptr(self.h)

    def close(self):
        if self.h:
            lib().mi_dl_csi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PbchResult(C.Structure):
    """mi_pbch_result_t"""
    _fields_ = [("found", C.c_uint32), ("nof_ports", C.c_uint32), ("sfn_offset", C.c_uint32),
                ("n_frames_used", C.c_uint32), ("bits", C.c_uint8 * 24)]


def pbch_re_indices(cell_id, nof_prb):
    """the 240 PBCH REs of a cell in mapping order (grid index l * 12 nof_prb + k); host only"""
    re = np.zeros(240, np.uint32)
    if lib().mi_pbch_re_indices(cell_id, nof_prb, re.ctypes.data):
        raise RuntimeError("mi_pbch_re_indices: " + last_error())
    return re


def tx_pbch(cell_id, nof_prb, nof_ports, bits24, phase, iq, h=None):
    """add the PBCH quarter `phase` of a BCH TTI carrying bits24 to a subframe-0 iq (float32 interleaved, in place)"""
    assert iq.dtype == np.float32 and iq.flags.c_contiguous and len(iq) >= 2 * lib().mi_sf_len(nof_prb)
    b = np.ascontiguousarray(bits24, np.uint8)
    assert b.size == 24
    hh = None
    if h is not None:
        hh = np.zeros(4, np.float32)
        for p, v in enumerate(h[:2]):
            hh[2 * p], hh[2 * p + 1] = v.real, v.imag
    if lib().mi_tx_pbch(cell_id, nof_prb, nof_ports, b.ctypes.data, phase, None if hh is None else hh.ctypes.data,
                        iq.ctypes.data):
        raise RuntimeError("mi_tx_pbch: " + last_error())


class Pbch:
    """PBCH receiver over a batch's grid / channel estimates (mi_pbch_*): every subframe 0 of the batch is a frame."""
    LLR, DECODE = 1, 2

    def __init__(self, batch):
        self.batch = batch
        self.h = lib().mi_pbch_create(batch.h)
        if not self.h:
            raise RuntimeError("mi_pbch_create: " + last_error())
        self.n_cand = 0

    @property
    def n_frames(self):
        return lib().mi_pbch_n_frames(self.h)

    @property
    def n_jobs(self):
        return lib().mi_pbch_n_jobs(self.h)

    def frame_of(self, sf):
        return lib().mi_pbch_frame_of(self.h, sf)

    def set_candidates(self, cands):
        """cands: per candidate the batch subframe indices of its 1..4 frames, oldest first"""
        sf = np.zeros((max(len(cands), 1), 4), np.uint32)
        n = np.zeros(max(len(cands), 1), np.uint32)
        for i, c in enumerate(cands):
            n[i] = len(c)
            sf[i, :min(len(c), 4)] = list(c)[:4]
        self.n_cand = 0
        if lib().mi_pbch_set_candidates(self.h, sf.ctypes.data, n.ctypes.data, len(cands)):
            raise RuntimeError("mi_pbch_set_candidates: " + last_error())
        self.n_cand = len(cands)

    def run(self, stream_ptr=None, mask=3):
        if lib().mi_pbch_run(self.h, mask, C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_pbch_run: " + last_error())

    def result(self, cand):
        """None, or (nof_ports, sfn_offset, n_frames_used, bits[24]) of the first decode that passed"""
        r = PbchResult()
        rc = lib().mi_pbch_result(self.h, cand, C.byref(r))
        if rc < 0:
            raise RuntimeError("mi_pbch_result: " + last_error())
        return (r.nof_ports, r.sfn_offset, r.n_frames_used, np.array(r.bits[:], np.uint8)) if rc == 1 else None

    def llr(self):
        """soft bits [frame][hypothesis][480], not descrambled"""
        n = lib().mi_pbch_llr_floats(self.h)
        out = np.zeros(n, np.float32)
        if n and lib().mi_pbch_llr(self.h, out.ctypes.data, n, 0):
            raise RuntimeError("mi_pbch_llr: " + last_error())
        return out.reshape(-1, 2, 480)

    def set_llr(self, host):
        a = np.ascontiguousarray(host, np.float32)
        if lib().mi_pbch_llr(self.h, a.ctypes.data, a.size, 1):
            raise RuntimeError("mi_pbch_llr: " + last_error())

    def close(self):
        if self.h:
            lib().mi_pbch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CellResult(C.Structure):
    """mi_cell_result_t"""
    _fields_ = [("found", C.c_uint32), ("cell_id", C.c_uint32), ("mode", C.c_float), ("peak", C.c_float),
                ("psr", C.c_float), ("cfo", C.c_float), ("sf_start", C.c_uint64)]


class CellSearch:
    """Cell search over device-resident 1.92 Msps IQ (mi_cellsearch_*): one result per N_ID_2."""
    HALF = 9600

    def __init__(self):
        self.h = lib().mi_cellsearch_create()
        if not self.h:
            raise RuntimeError("mi_cellsearch_create: " + last_error())

    def run(self, d_iq, offsets, threshold=0.0, stream_ptr=None):
        off = np.ascontiguousarray(offsets, np.uint64)
        out = (CellResult * 3)()
        if lib().mi_cellsearch_run(self.h, C.c_void_p(d_iq), off.ctypes.data, len(off), threshold, out,
                                   C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_cellsearch_run: " + last_error())
        return [dict(found=bool(r.found), cell_id=r.cell_id, mode=r.mode, peak=r.peak, psr=r.psr, cfo=r.cfo,
                     sf_start=r.sf_start) for r in out]

    def close(self):
        if self.h:
            lib().mi_cellsearch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mib(C.Structure):
    """mi_mib_t"""
    _fields_ = [(n, C.c_uint32) for n in ("nof_prb", "nof_ports", "phich_length", "phich_resources", "sfn", "n_frames")] + \
               [("sf_start", C.c_uint64), ("bits", C.c_uint8 * 24)]


class Timestamp(C.Structure):
    """srslte_timestamp_t"""
    _fields_ = [("full_secs", C.c_long), ("frac_secs", C.c_double)]


RECV_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(Timestamp))


class Acq:
    """Streaming acquisition over a receive callback at 1.92 Msps (mi_acq_*).  recv(n) returns n cf32 samples as
    a float32 array of 2 n values, or None when the stream has ended."""

    def __init__(self, recv):
        def cb(handler, data, nsamples, ts):
            x = recv(nsamples)
            if x is None or len(x) < 2 * nsamples:
                return -1
            x = np.ascontiguousarray(x[:2 * nsamples], np.float32)
            C.memmove(data, x.ctypes.data, 8 * nsamples)
            return nsamples
        self._cb = RECV_CB(cb)           # kept alive as long as the instance
        self.h = lib().mi_acq_create(C.cast(self._cb, C.c_void_p), None)
        if not self.h:
            raise RuntimeError("mi_acq_create: " + last_error())

    def search(self, n_half_frames, threshold=0.0):
        """(results per N_ID_2 as CellSearch.run, best N_ID_2 or None)"""
        out = (CellResult * 3)()
        best = C.c_uint32()
        rc = lib().mi_acq_search(self.h, n_half_frames, threshold, out, C.byref(best))
        if rc < 0:
            raise RuntimeError("mi_acq_search: " + last_error())
        res = [dict(found=bool(r.found), cell_id=r.cell_id, mode=r.mode, peak=r.peak, psr=r.psr, cfo=r.cfo,
                    sf_start=r.sf_start) for r in out]
        return res, (best.value if rc > 0 else None)

    def mib(self, cell_id, cfo, max_frames):
        """the Mib found within max_frames radio frames, or None"""
        m = Mib()
        rc = lib().mi_acq_mib(self.h, cell_id, cfo, max_frames, C.byref(m))
        if rc < 0:
            raise RuntimeError("mi_acq_mib: " + last_error())
        return m if rc == 1 else None

    def close(self):
        if self.h:
            lib().mi_acq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PssResult(C.Structure):
    _fields_ = [("nid2", C.c_uint32), ("lag", C.c_uint32), ("rho", C.c_float), ("cfo", C.c_float)]


class SssResult(C.Structure):
    _fields_ = [("nid1", C.c_uint32), ("sf5", C.c_uint32), ("score", C.c_float)]


def tx_sync(cell_id, nof_prb, sf_idx, iq, amp=1.0):
    """add the PSS / SSS of subframe 0 / 5 to iq (float32 interleaved, in place)"""
    assert iq.dtype == np.float32 and iq.flags.c_contiguous
    rc = lib().mi_tx_sync(cell_id, nof_prb, sf_idx, amp, iq.ctypes.data)
    if rc < 0:
        raise RuntimeError("mi_tx_sync: " + last_error())
    return rc


class Sync:
    """Sync front end (mi_sync_*) over device-resident IQ (offsets in cf32 samples)."""

    def __init__(self, nof_prb):
        self.h = lib().mi_sync_create(nof_prb)
        if not self.h:
            raise RuntimeError("mi_sync_create: " + last_error())
        self.N = lib().mi_sync_fft_size(self.h)

    def pss(self, d_iq, offsets, nlag, nid2_mask=7, stream_ptr=None):
        off = np.ascontiguousarray(offsets, np.uint64)
        out = (PssResult * max(len(off), 1))()
        if lib().mi_sync_pss(self.h, C.c_void_p(d_iq), off.ctypes.data, len(off), nlag, nid2_mask, out,
                             C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_sync_pss: " + last_error())
        return [(r.nid2, r.lag, r.rho, r.cfo) for r in out[:len(off)]]

    def sss(self, d_iq, sf_offsets, nid2, cfo, stream_ptr=None):
        off = np.ascontiguousarray(sf_offsets, np.uint64)
        n2 = np.ascontiguousarray(nid2, np.uint32)
        cf = np.ascontiguousarray(cfo, np.float32)
        out = (SssResult * max(len(off), 1))()
        if lib().mi_sync_sss(self.h, C.c_void_p(d_iq), off.ctypes.data, n2.ctypes.data, cf.ctypes.data, len(off), out,
                             C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_sync_sss: " + last_error())
        return [(r.nid1, r.sf5, r.score) for r in out[:len(off)]]

    def correct(self, d_src, src_off, d_dst, dst_off, cfo, length, stream_ptr=None):
        a = np.ascontiguousarray(src_off, np.uint64)
        b = np.ascontiguousarray(dst_off, np.uint64)
        c = np.ascontiguousarray(cfo, np.float32)
        if lib().mi_sync_correct(self.h, C.c_void_p(d_src), a.ctypes.data, C.c_void_p(d_dst), b.ctypes.data,
                                 c.ctypes.data, len(a), length, C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_sync_correct: " + last_error())

    def close(self):
        if self.h:
            lib().mi_sync_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """Page-locked host memory (mi_host_alloc) viewed as a numpy array."""

    def __init__(self, nbytes, dtype=np.float32):
        self.ptr = lib().mi_host_alloc(nbytes)
        if not self.ptr:
            raise RuntimeError("mi_host_alloc: " + last_error())
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self.ptr)).view(dtype)

    def close(self):
        if self.ptr:
            self.array = None
            lib().mi_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipe:
    """Double-buffered host-IQ pipeline (mi_dl_pipe_*): submit() returns a slot without blocking."""

    def __init__(self, cfgs, max_its=4, profile=False, tdec_i16=True, iq_sc16=False, n_rx=1, keep_llr=False):
        """n_rx: receive antennas; submit() then copies the n_rx IQ planes of the host buffer"""
        self.cfgs = list(cfgs)
        self._arr = cfg_array(self.cfgs)
        flags = (FLAG_PROFILE if profile else 0) | (FLAG_TDEC_I16 if tdec_i16 else FLAG_TDEC_GEN) | \
            (FLAG_IQ_SC16 if iq_sc16 else 0) | (FLAG_KEEP_LLR if keep_llr else 0)
        arr = C.cast(self._arr, C.c_void_p)
        self.h = lib().mi_dl_pipe_create(arr, len(self.cfgs), max_its, flags) if n_rx == 1 else \
            lib().mi_dl_pipe_create_rx(arr, len(self.cfgs), n_rx, max_its, flags)
        if not self.h:
            raise RuntimeError("mi_dl_pipe_create: " + last_error())

    def submit(self, host_ptr):
        s = lib().mi_dl_pipe_submit(self.h, C.c_void_p(host_ptr))
        if s < 0:
            raise RuntimeError("mi_dl_pipe_submit: " + last_error())
        return s

    def wait(self, slot):
        if lib().mi_dl_pipe_wait(self.h, slot):
            raise RuntimeError("mi_dl_pipe_wait: " + last_error())

    def batch(self, slot):
        return Batch.view(lib().mi_dl_pipe_batch(self.h, slot), self.cfgs)

    def close(self):
        if self.h:
            lib().mi_dl_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SC16_GAIN = 0.25   # receive gain before sc16 quantisation: the synthetic TX peaks at ~2.5 (a radio's AGC
                   # keeps samples inside [-1, 1)); a power of two, so gain * x is exact


def to_sc16(iq_f32, gain=SC16_GAIN):
    """fc32 interleaved I/Q -> UHD sc16 (gain, round to nearest, saturate): FLAG_IQ_SC16's wire format."""
    return np.clip(np.rint(np.asarray(iq_f32, np.float32) * (gain * 32768.0)), -32768, 32767).astype(np.int16)


def turbo_encode(bits, K, F=0):
    """36.212 turbo encoder of the product (host): 3(K+4) values in triplet order, 2 = <NULL>."""
    d = np.zeros(3 * (K + 4), np.uint8)
    b = np.ascontiguousarray(bits, np.uint8)
    if lib().mi_turbo_encode(b.ctypes.data, K, F, d.ctypes.data):
        raise RuntimeError("mi_turbo_encode failed")
    return d


class TdecBatch:
    """Raw code-block turbo decoding (mi_tdec_*, the srslte_tdec_* / turbodecoder_test contract)."""

    def __init__(self, K, n_cb, max_its=8, early_stop=False, crc24a=False, profile=False, tdec_i16=True, sched=None):
        self.K, self.n_cb = K, n_cb
        flags = (FLAG_PROFILE if profile else 0) | (FLAG_TDEC_I16 if tdec_i16 else FLAG_TDEC_GEN) | SCHED_FLAGS[sched]
        self.h = lib().mi_tdec_create(K, n_cb, max_its, int(early_stop), int(crc24a), flags)
        if not self.h:
            raise RuntimeError("mi_tdec_create: " + last_error())

    def run(self, d_in_ptr, stream_ptr=None):
        if lib().mi_tdec_run(self.h, C.c_void_p(d_in_ptr), C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_tdec_run: " + last_error())

    def results(self):
        bits = np.zeros(self.n_cb * self.K // 8, np.uint8)
        its = np.zeros(self.n_cb, np.uint32)
        ok = np.zeros(self.n_cb, np.uint32)
        if lib().mi_tdec_download(self.h, bits.ctypes.data, its.ctypes.data, ok.ctypes.data):
            raise RuntimeError("mi_tdec_download: " + last_error())
        return np.unpackbits(bits).reshape(self.n_cb, self.K), its, ok

    def stage_ms(self):
        ms = np.zeros(len(STAGES), np.float32)
        n = C.c_uint32(0)
        if lib().mi_tdec_stage_ms(self.h, ms.ctypes.data, C.byref(n)):
            raise RuntimeError("stage_ms: " + last_error())
        return dict(zip(STAGES, ms.tolist())), n.value

    def profile_reset(self):
        lib().mi_tdec_profile_reset(self.h)

    def algo_bytes(self):
        return lib().mi_tdec_algo_bytes(self.h)

    @property
    def turbo_win(self):
        return lib().mi_tdec_turbo_win(self.h) == 1

    @property
    def turbo_sched(self):
        return {1: "win", 2: "lanex", 3: "lanexr", 4: "p2"}.get(lib().mi_tdec_turbo_win(self.h), "lane")

    def close(self):
        if self.h:
            lib().mi_tdec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pdsch_G(cfg):
    return lib().mi_pdsch_G(C.byref(cfg))


# ---- UL PUSCH transmitter (include/mi_ul.h) ---------------------------------------
UL_STAGES = ("crc", "encode", "mod")


class UlCfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("cell_id", "nof_prb", "sf_idx", "rnti", "n_prb", "L_prb", "tbs", "Qm", "rv",
                                          "group_hopping", "sequence_hopping", "delta_ss", "cyclic_shift", "n_dmrs2",
                                          "ack_len", "ack", "I_offset_ack", "hop", "n_prb1", "cqi_len",
                                          "I_offset_cqi")] + [("cqi", C.c_uint8 * 64)] + \
        [(n, C.c_uint32) for n in ("ri_len", "ri", "I_offset_ri", "n_srs", "n_symb_initial")]


class UlRes(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_symb", "G", "q_ack", "q_ri", "q_cqi", "C")] + [("E", C.c_uint32 * 16)]


PUSCH_SRS_OFF, PUSCH_SRS_OVERLAP, PUSCH_SRS_ALL_CS = range(3)


def ul_cfg(cell_id=1, nof_prb=100, sf_idx=1, rnti=0x46, n_prb=0, L_prb=100, tbs=0, Qm=4, rv=0, gh=0, sh=0, dss=0,
           cs=0, n2=0, ack_len=0, ack=0, ioff=0, n_prb1=None, cqi=(), cqi_ioff=2, ri_len=0, ri=0, ri_ioff=0, n_srs=0,
           n_symb_initial=0):
    """n_prb1: start PRB of slot 1 (frequency hopping), None = no hopping; cqi: CQI bits o_0.. (36.212
    5.2.2.6.4) with beta_offset index cqi_ioff; ri_len / ri / ri_ioff: RI on PUSCH; n_srs = 1: the last symbol is left
    to the SRS (11 data symbols); n_symb_initial: N_symb^PUSCH-initial of the Q' formulas, 0 = 12 - n_srs"""
    hop, n1 = (0, 0) if n_prb1 is None else (1, n_prb1)
    c = UlCfg(cell_id, nof_prb, sf_idx, rnti, n_prb, L_prb, tbs, Qm, rv, gh, sh, dss, cs, n2, ack_len, ack, ioff,
              hop, n1, len(cqi), cqi_ioff)
    for i, b in enumerate(cqi):
        c.cqi[i] = b
    c.ri_len, c.ri, c.I_offset_ri = ri_len, ri, ri_ioff
    c.n_srs, c.n_symb_initial = n_srs, n_symb_initial
    return c


def ul_pusch_resource(cfg):
    """mi_ul_pusch_resource: the planned UlRes (n_symb, G, Q' values, C, E[]); raises on a rejected configuration"""
    r = UlRes()
    if lib().mi_ul_pusch_resource(C.byref(cfg), C.byref(r)):
        raise RuntimeError("mi_ul_pusch_resource: " + last_error())
    return r


def ul_pusch_n_srs(nof_prb, srs_subframe_config, srs_bw_cfg, sf_idx, n_prb0, n_prb1, L_prb, ue_sends_srs=0,
                   rule=PUSCH_SRS_OVERLAP):
    """mi_ul_pusch_n_srs: 1 if the PUSCH leaves the last symbol to the SRS, 0 if not, -1 for bad arguments"""
    return lib().mi_ul_pusch_n_srs(nof_prb, srs_subframe_config, srs_bw_cfg, sf_idx, n_prb0, n_prb1, L_prb,
                                   int(ue_sends_srs), rule)


class UlBatch:
    """Owns one mi_ul_batch_t: N PUSCH transmissions planned once; run() enqueues the chain."""

    def __init__(self, cfgs, profile=False):
        self.cfgs = list(cfgs)
        self._arr = (UlCfg * len(self.cfgs))(*self.cfgs)
        self.h = lib().mi_ul_batch_create(C.cast(self._arr, C.c_void_p), len(self.cfgs), 1 if profile else 0)
        if not self.h:
            raise RuntimeError("mi_ul_batch_create: " + last_error())

    def close(self):
        if self.h:
            lib().mi_ul_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def payload_bytes(self):
        return lib().mi_ul_batch_payload_bytes(self.h)

    @property
    def iq_samples(self):
        return lib().mi_ul_batch_iq_samples(self.h)

    @property
    def n_codeblocks(self):
        return lib().mi_ul_batch_n_codeblocks(self.h)

    def payload_offset(self, i):
        return lib().mi_ul_batch_payload_offset(self.h, i)

    def iq_offset(self, i):
        return lib().mi_ul_batch_iq_offset(self.h, i)

    def run(self, d_payload_ptr, d_iq_ptr, stream_ptr=None):
        if lib().mi_ul_batch_run(self.h, C.c_void_p(d_payload_ptr), C.c_void_p(d_iq_ptr), C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_ul_batch_run: " + last_error())

    def symbols(self, i):
        c = self.cfgs[i]
        out = np.zeros((12 - c.n_srs) * 12 * c.L_prb, np.uint8)   # g, then the Q'_RI cells as zeros
        if lib().mi_ul_batch_symbols(self.h, i, out.ctypes.data):
            raise RuntimeError("mi_ul_batch_symbols: " + last_error())
        return out

    def stage_ms(self):
        ms = np.zeros(len(UL_STAGES), np.float32)
        n = C.c_uint32(0)
        if lib().mi_ul_batch_stage_ms(self.h, ms.ctypes.data, C.byref(n)):
            raise RuntimeError("mi_ul_batch_stage_ms: " + last_error())
        return dict(zip(UL_STAGES, ms.tolist())), n.value

    def profile_reset(self):
        lib().mi_ul_batch_profile_reset(self.h)

    def algo_bytes(self):
        return lib().mi_ul_batch_algo_bytes(self.h)


# ---- PUCCH formats 1/1a/1b, 2/2a/2b (include/mi_ul.h) -----------------------------------------------
PUCCH_1, PUCCH_1A, PUCCH_1B, PUCCH_2, PUCCH_2A, PUCCH_2B = range(6)
PUCCH_CFG_FIELDS = ("cell_id", "nof_prb", "sf_idx", "rnti", "format", "n_pucch", "delta_shift", "N_cs", "n_rb_2",
                    "group_hopping", "shortened", "cqi_len")


class PucchCfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in PUCCH_CFG_FIELDS]


class PucchRes(C.Structure):
    _fields_ = [("n_prb", C.c_uint32 * 2), ("u", C.c_uint32 * 2), ("n_prime", C.c_uint32 * 2),
                ("n_oc", C.c_uint32 * 2), ("n_cs", (C.c_uint32 * 7) * 2)]


# the same layouts as numpy records, for mi_pucch_resource_n over arrays of configurations
PUCCH_CFG_DTYPE = np.dtype([(n, np.uint32) for n in PUCCH_CFG_FIELDS])
PUCCH_RES_DTYPE = np.dtype([("n_prb", np.uint32, 2), ("u", np.uint32, 2), ("n_prime", np.uint32, 2),
                            ("n_oc", np.uint32, 2), ("n_cs", np.uint32, (2, 7))])


def pucch_cfg(cell_id=1, nof_prb=6, sf_idx=0, rnti=0x46, format=PUCCH_1A, n_pucch=0, delta_shift=1, N_cs=0, n_rb_2=0,
              group_hopping=0, shortened=0, cqi_len=0):
    return PucchCfg(cell_id, nof_prb, sf_idx, rnti, format, n_pucch, delta_shift, N_cs, n_rb_2, group_hopping,
                    shortened, cqi_len)


def pucch_uci(ack=0, cqi=()):
    """the UCI word of one transmission: HARQ-ACK bits 0-1 (bit 0 = first), CQI bits o_0.. at bits 8.."""
    w = ack & 3
    for k, b in enumerate(cqi):
        w |= (int(b) & 1) << (8 + k)
    return w


def pucch_resource(cfg):
    """mi_pucch_resource: the planned PucchRes; raises on a rejected configuration"""
    r = PucchRes()
    if lib().mi_pucch_resource(C.byref(cfg), C.byref(r)):
        raise RuntimeError("mi_pucch_resource: " + last_error())
    return r


def pucch_resource_n(cfgs):
    """mi_pucch_resource_n over a PUCCH_CFG_DTYPE array: (records planned before the first rejection, their count)"""
    cfgs = np.ascontiguousarray(cfgs, PUCCH_CFG_DTYPE)
    out = np.zeros(len(cfgs), PUCCH_RES_DTYPE)
    n = lib().mi_pucch_resource_n(cfgs.ctypes.data, len(cfgs), out.ctypes.data)
    return out[:n], n


def pucch_select(ack_len=0, sr=False, cqi_len=0, simul_cqi_ack_dropped=False, n_cce=0, N_pucch_1=0, n_pucch_2=0,
                 n_pucch_sr=0):
    """mi_pucch_select: (format, n_pucch), or None when there is nothing to send"""
    n = C.c_uint32(0)
    f = lib().mi_pucch_select(ack_len, int(sr), cqi_len, int(simul_cqi_ack_dropped), n_cce, N_pucch_1, n_pucch_2,
                              n_pucch_sr, C.byref(n))
    return None if f < 0 else (f, n.value)


class _TxBatch:
    """Owns one mi_<PREFIX>_batch_t of N transmissions planned once from CFG records; resource() returns a RES."""
    PREFIX = CFG = RES = None

    def __init__(self, cfgs, flags=0):
        self.cfgs = list(cfgs)
        self._arr = (self.CFG * len(self.cfgs))(*self.cfgs)
        self.h = self._fn("create")(C.cast(self._arr, C.c_void_p), len(self.cfgs), flags)
        if not self.h:
            raise RuntimeError(f"mi_{self.PREFIX}_batch_create: " + last_error())

    def _fn(self, name):
        return getattr(lib(), f"mi_{self.PREFIX}_batch_{name}")

    def close(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def iq_samples(self):
        return self._fn("iq_samples")(self.h)

    def iq_offset(self, i):
        return self._fn("iq_offset")(self.h, i)

    def resource(self, i):
        r = self.RES()
        if self._fn("resource")(self.h, i, C.byref(r)):
            raise RuntimeError(f"mi_{self.PREFIX}_batch_resource: " + last_error())
        return r

    def _run_cfo_scale(self, d_iq_ptr, stream_ptr, d_cfo_ptr, d_scale_ptr):
        if self._fn("run")(self.h, C.c_void_p(d_cfo_ptr or 0), C.c_void_p(d_scale_ptr or 0), C.c_void_p(d_iq_ptr),
                           C.c_void_p(stream_ptr or 0)):
            raise RuntimeError(f"mi_{self.PREFIX}_batch_run: " + last_error())


class PucchBatch(_TxBatch):
    """Owns one mi_pucch_batch_t: N PUCCH transmissions planned once; run() encodes them from device UCI words."""
    PREFIX, CFG, RES = "pucch", PucchCfg, PucchRes

    def __init__(self, cfgs):
        super().__init__(cfgs, 0)

    def run(self, d_uci_ptr, d_iq_ptr, stream_ptr=None):
        if lib().mi_pucch_batch_run(self.h, C.c_void_p(d_uci_ptr), C.c_void_p(d_iq_ptr), C.c_void_p(stream_ptr or 0)):
            raise RuntimeError("mi_pucch_batch_run: " + last_error())


# ---- PRACH preamble, formats 0-3 (include/mi_ul.h) --------------------------------------------------
PRACH_FLAG_SINGLE_RESIDUE = 1
PRACH_CFG_FIELDS = ("nof_prb", "config_idx", "root_seq_idx", "zero_corr_zone", "high_speed", "freq_offset",
                    "preamble_idx")
PRACH_RES_FIELDS = ("format", "N_ifft", "N_cp", "N_seq", "N_cs", "u", "C_v", "first_bin", "n_roots")


class PrachCfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in PRACH_CFG_FIELDS]


class PrachRes(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in PRACH_RES_FIELDS]


# the same layouts as numpy records, for mi_prach_resource_n over arrays of configurations
PRACH_CFG_DTYPE = np.dtype([(n, np.uint32) for n in PRACH_CFG_FIELDS])
PRACH_RES_DTYPE = np.dtype([(n, np.uint32) for n in PRACH_RES_FIELDS])


def prach_cfg(nof_prb=6, config_idx=0, root_seq_idx=0, zero_corr_zone=0, high_speed=0, freq_offset=0, preamble_idx=0):
    return PrachCfg(nof_prb, config_idx, root_seq_idx, zero_corr_zone, high_speed, freq_offset, preamble_idx)


def prach_resource(cfg):
    """mi_prach_resource: the planned PrachRes; raises on a rejected configuration"""
    r = PrachRes()
    if lib().mi_prach_resource(C.byref(cfg), C.byref(r)):
        raise RuntimeError("mi_prach_resource: " + last_error())
    return r


def prach_resource_n(cfgs):
    """mi_prach_resource_n over a PRACH_CFG_DTYPE array: (records planned before the first rejection, their count)"""
    cfgs = np.ascontiguousarray(cfgs, PRACH_CFG_DTYPE)
    out = np.zeros(len(cfgs), PRACH_RES_DTYPE)
    n = lib().mi_prach_resource_n(cfgs.ctypes.data, len(cfgs), out.ctypes.data)
    return out[:n], n


def prach_root(logical_idx):
    """mi_prach_root: the physical root of a logical index (Table 5.7.2-4), -1 beyond 837"""
    return lib().mi_prach_root(logical_idx)


def prach_format(config_idx):
    """mi_prach_format: 0..3, -1 for the N/A rows"""
    return lib().mi_prach_format(config_idx)


def prach_send_tti(config_idx, tti, allowed_subframe=-1):
    return lib().mi_prach_send_tti(config_idx, tti, allowed_subframe)


class PrachBatch(_TxBatch):
    """Owns one mi_prach_batch_t: N preambles planned once; run() generates them into device IQ."""
    PREFIX, CFG, RES = "prach", PrachCfg, PrachRes

    def run(self, d_iq_ptr, stream_ptr=None, d_cfo_ptr=None, d_scale_ptr=None):
        self._run_cfo_scale(d_iq_ptr, stream_ptr, d_cfo_ptr, d_scale_ptr)


# ---- SRS, periodic (include/mi_ul.h) ----------------------------------------------------------------
SRS_FLAG_LAST_SYMBOL_ONLY = 1
SRS_CFG_FIELDS = ("cell_id", "nof_prb", "tti", "bw_cfg", "B", "b_hop", "n_rrc", "k_tc", "n_srs", "I_srs",
                  "group_hopping", "sequence_hopping", "delta_ss")


class SrsCfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in SRS_CFG_FIELDS]


class SrsRes(C.Structure):
    _fields_ = [("m_srs", C.c_uint32), ("M_sc", C.c_uint32), ("k0", C.c_uint32), ("n_b", C.c_uint32 * 4)] + \
        [(n, C.c_uint32) for n in ("n_SRS", "T_srs", "u", "v", "nzc", "q", "n_cs")]


# the same layouts as numpy records, for mi_srs_resource_n over arrays of configurations
SRS_CFG_DTYPE = np.dtype([(n, np.uint32) for n in SRS_CFG_FIELDS])
SRS_RES_DTYPE = np.dtype([("m_srs", np.uint32), ("M_sc", np.uint32), ("k0", np.uint32), ("n_b", np.uint32, 4)] +
                         [(n, np.uint32) for n in ("n_SRS", "T_srs", "u", "v", "nzc", "q", "n_cs")])


def srs_cfg(cell_id=1, nof_prb=6, tti=0, bw_cfg=7, B=0, b_hop=3, n_rrc=0, k_tc=0, n_srs=0, I_srs=0, group_hopping=0,
            sequence_hopping=0, delta_ss=0):
    return SrsCfg(cell_id, nof_prb, tti, bw_cfg, B, b_hop, n_rrc, k_tc, n_srs, I_srs, group_hopping, sequence_hopping,
                  delta_ss)


def srs_resource(cfg):
    """mi_srs_resource: the planned SrsRes; raises on a rejected configuration"""
    r = SrsRes()
    if lib().mi_srs_resource(C.byref(cfg), C.byref(r)):
        raise RuntimeError("mi_srs_resource: " + last_error())
    return r


def srs_resource_n(cfgs):
    """mi_srs_resource_n over a SRS_CFG_DTYPE array: (records planned before the first rejection, their count)"""
    cfgs = np.ascontiguousarray(cfgs, SRS_CFG_DTYPE)
    out = np.zeros(len(cfgs), SRS_RES_DTYPE)
    n = lib().mi_srs_resource_n(cfgs.ctypes.data, len(cfgs), out.ctypes.data)
    return out[:n], n


class SrsBatch(_TxBatch):
    """Owns one mi_srs_batch_t: N SRS transmissions planned once; run() encodes them into device IQ."""
    PREFIX, CFG, RES = "srs", SrsCfg, SrsRes

    def run(self, d_iq_ptr, stream_ptr=None, d_cfo_ptr=None, d_scale_ptr=None):
        self._run_cfo_scale(d_iq_ptr, stream_ptr, d_cfo_ptr, d_scale_ptr)


# ---- open-loop UL power control (include/mi_ul.h), host only ----------------------------------------
P_CMAX = 23.0


class UlPowerCfg(C.Structure):
    _fields_ = [("p0_nominal_pusch", C.c_float), ("alpha", C.c_float), ("p0_nominal_pucch", C.c_float),
                ("delta_f_pucch", C.c_float * 5), ("delta_preamble_msg3", C.c_float), ("p0_ue_pusch", C.c_float),
                ("delta_mcs_based", C.c_uint32), ("acc_enabled", C.c_uint32), ("p0_ue_pucch", C.c_float),
                ("p_srs_offset", C.c_float)]


def ul_power_cfg(p0_nominal_pusch=-80.0, alpha=0.8, p0_nominal_pucch=-100.0, delta_f_pucch=(0.0, 1.0, 0.0, 0.0, 2.0),
                 delta_preamble_msg3=4.0, p0_ue_pusch=0.0, delta_mcs_based=0, acc_enabled=0, p0_ue_pucch=0.0,
                 p_srs_offset=7.0):
    return UlPowerCfg(p0_nominal_pusch, alpha, p0_nominal_pucch, (C.c_float * 5)(*delta_f_pucch), delta_preamble_msg3,
                      p0_ue_pusch, int(delta_mcs_based), int(acc_enabled), p0_ue_pucch, p_srs_offset)


def ul_pusch_power(cfg, PL, p0_preamble=0.0, L_prb=1, sum_Kr=0):
    """mi_ul_pusch_power (36.213 5.1.1.1), dBm"""
    return lib().mi_ul_pusch_power(C.byref(cfg), PL, p0_preamble, L_prb, sum_Kr)


def ul_pusch_power_nsymb(cfg, PL, p0_preamble=0.0, L_prb=1, sum_Kr=0, n_symb_initial=12):
    """mi_ul_pusch_power_nsymb: mi_ul_pusch_power with N_RE = 12 L_prb n_symb_initial, dBm"""
    return lib().mi_ul_pusch_power_nsymb(C.byref(cfg), PL, p0_preamble, L_prb, sum_Kr, n_symb_initial)


def ul_pucch_power(cfg, PL, format=PUCCH_1A, n_cqi=0, n_harq=0):
    """mi_ul_pucch_power (36.213 5.1.2.1), dBm"""
    return lib().mi_ul_pucch_power(C.byref(cfg), PL, format, n_cqi, n_harq)


def ul_srs_power(cfg, PL, m_srs=4):
    """mi_ul_srs_power (36.213 5.1.3.1), dBm"""
    return lib().mi_ul_srs_power(C.byref(cfg), PL, m_srs)
