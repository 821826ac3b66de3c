"""DCI formats 2 and 2A restated from 3GPP TS 36.212 5.3.3.1.5 / 5.3.3.1.5A (FDD, 2 antenna ports) and the type 0 /
type 1 resource allocations of 36.213 7.1.6.1 / 7.1.6.2, in integer Python: the reference test_dci2_ref.py holds the
C functions mi_dci_dl2_* to.  Written from the specification, independent of srsue_amd/csrc.

A grant is a dict: format ("2" / "2A"), alloc_type, type0_alloc, type1_subset, type1_shift, type1_bitmap, tpc, harq,
swap, tb = [(mcs, ndi, rv), (mcs, ndi, rv)], pinfo."""

AMBIGUOUS = (12, 14, 16, 20, 24, 26, 32, 40, 44, 56)   # 36.212 Table 5.3.3.1.2-1


def rbg_size(n_rb):
    """P of 36.213 Table 7.1.6.1-1"""
    return 1 if n_rb <= 10 else 2 if n_rb <= 26 else 3 if n_rb <= 63 else 4


def ceil_log2(x):
    return (x - 1).bit_length()


def widths(fmt, n_rb):
    """field widths in transmission order: header, resource block assignment, then the fixed fields"""
    P = rbg_size(n_rb)
    return dict(hdr=1 if n_rb > 10 else 0, rba=-(-n_rb // P), tpc=2, harq=3, swap=1, tb=8, pinfo=3 if fmt == "2" else 0)


def size(fmt, n_rb):
    w = widths(fmt, n_rb)
    n = w["hdr"] + w["rba"] + w["tpc"] + w["harq"] + w["swap"] + 2 * w["tb"] + w["pinfo"]
    return n + 1 if n in AMBIGUOUS else n


def _bits(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def _val(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v


def pack(n_rb, g):
    w = widths(g["format"], n_rb)
    P = rbg_size(n_rb)
    out = []
    if w["hdr"]:
        out += [g["alloc_type"]]
    if g["alloc_type"] == 0:
        out += _bits(g["type0_alloc"], w["rba"])
    else:
        n1 = w["rba"] - ceil_log2(P) - 1
        out += _bits(g["type1_subset"], ceil_log2(P)) + [g["type1_shift"]] + _bits(g["type1_bitmap"], n1)
    out += _bits(g["tpc"], 2) + _bits(g["harq"], 3) + [g["swap"]]
    for mcs, ndi, rv in g["tb"]:
        out += _bits(mcs, 5) + [ndi] + _bits(rv, 2)
    out += _bits(g["pinfo"], w["pinfo"])
    return out + [0] * (size(g["format"], n_rb) - len(out))


def unpack(fmt, n_rb, bits):
    assert len(bits) == size(fmt, n_rb)
    w = widths(fmt, n_rb)
    P = rbg_size(n_rb)
    pos = [0]

    def take(n):
        v = _val(bits[pos[0]:pos[0] + n])
        pos[0] += n
        return v
    g = dict(format=fmt, alloc_type=take(1) if w["hdr"] else 0, type0_alloc=0, type1_subset=0, type1_shift=0,
             type1_bitmap=0)
    if g["alloc_type"] == 0:
        g["type0_alloc"] = take(w["rba"])
    else:
        g["type1_subset"], g["type1_shift"] = take(ceil_log2(P)), take(1)
        g["type1_bitmap"] = take(w["rba"] - ceil_log2(P) - 1)
    g["tpc"], g["harq"], g["swap"] = take(2), take(3), take(1)
    g["tb"] = [(take(5), take(1), take(2)) for _ in range(2)]
    g["pinfo"] = take(w["pinfo"])
    return g


def tb_enabled(tb):
    """a transport block is disabled by I_MCS = 0 and rv_idx = 1 (36.212 5.3.3.1.5)"""
    return not (tb[0] == 0 and tb[2] == 1)


def alloc_prbs(n_rb, g):
    """the allocated PRB indices (sorted), or None for a bitmap bit that addresses no VRB of the subset"""
    P = rbg_size(n_rb)
    n_rbg = -(-n_rb // P)
    if g["alloc_type"] == 0:       # 7.1.6.1: bit for RBG 0 is the MSB; the last RBG may be smaller
        return [p for r in range(n_rbg) if (g["type0_alloc"] >> (n_rbg - 1 - r)) & 1 for p in range(r * P, min((r + 1) * P, n_rb))]
    # 7.1.6.2
    p = g["type1_subset"]
    n_type1 = n_rbg - ceil_log2(P) - 1
    last = ((n_rb - 1) // P) % P
    n_subset = (n_rb - 1) // (P * P) * P + (P if p < last else (n_rb - 1) % P + 1 if p == last else 0)
    shift = n_subset - n_type1 if g["type1_shift"] else 0
    out = []
    for i in range(n_type1):
        if (g["type1_bitmap"] >> (n_type1 - 1 - i)) & 1:
            j = i + shift
            vrb = (j // P) * P * P + p * P + j % P
            if j >= n_subset or vrb >= n_rb:
                return None
            out.append(vrb)
    return sorted(out)


def random_grant(rng, fmt, n_rb, alloc_type=None, disable=None, swap=None):
    """a valid grant (a non-empty allocation that addresses VRBs of its subset); disable: 0 / 1 = that TB disabled"""
    P = rbg_size(n_rb)
    n_rbg = -(-n_rb // P)
    at = alloc_type if alloc_type is not None else (int(rng.integers(0, 2)) if n_rb > 10 else 0)
    while True:
        g = dict(format=fmt, alloc_type=at, type0_alloc=0, type1_subset=0, type1_shift=0, type1_bitmap=0,
                 tpc=int(rng.integers(0, 4)), harq=int(rng.integers(0, 8)),
                 swap=int(rng.integers(0, 2)) if swap is None else swap,
                 tb=[(int(rng.integers(0, 29)), int(rng.integers(0, 2)), int(rng.integers(0, 4))) for _ in range(2)],
                 pinfo=int(rng.integers(0, 8)) if fmt == "2" else 0)
        if at == 0:
            g["type0_alloc"] = int(rng.integers(1, 1 << n_rbg))
        else:
            g["type1_subset"] = int(rng.integers(0, P))
            g["type1_shift"] = int(rng.integers(0, 2))
            g["type1_bitmap"] = int(rng.integers(1, 1 << (n_rbg - ceil_log2(P) - 1)))
        for t in range(2):
            if disable == t:
                g["tb"][t] = (0, g["tb"][t][1], 1)
            elif not tb_enabled(g["tb"][t]):
                g["tb"][t] = (g["tb"][t][0], g["tb"][t][1], 0)
        if alloc_prbs(n_rb, g):
            return g
