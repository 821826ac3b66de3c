"""Independent numpy reference of the PRACH preamble (36.211 5.7; FDD, formats 0-3, N_ZC = 839): its own statement of
Tables 5.7.1-2, 5.7.2-2 and 5.7.2-4 and of the cyclic-shift formulas, the baseband signal of 5.7.3 computed the long
way (np.fft.fft of x_{u,v}, the 839 bins placed in an N_ifft-point grid, one np.fft.ifft in float64, CP, repetition,
frequency shift), and a correlation detector.  Nothing here calls the product or splits the transform."""
import functools

import numpy as np

NZC = 839
NFFT = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}
CP_TS = (3168, 21024, 6240, 21024)      # T_CP in T_s (30.72 MHz) per format
REPS = (1, 1, 2, 2)                      # T_SEQ / 24576 T_s
NCS_UNRESTRICTED = (0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419)
NCS_RESTRICTED = (15, 18, 22, 26, 32, 38, 46, 55, 68, 82, 100, 128, 158, 202, 237)

# Table 5.7.2-4 by groups "first-last logical index: u of every pair" (each u is followed by 839 - u)
ROOT_GROUPS = """
0-23:    129 140 120 210 168 84 105 93 70 60 2 1
24-29:   56 112 148
30-35:   80 42 40
36-41:   35 73 146
42-51:   31 28 30 27 29
52-63:   24 48 68 74 178 136
64-75:   86 78 43 39 20 21
76-89:   95 202 190 181 137 125 151
90-115:  217 128 142 122 203 118 110 89 103 61 55 15 14
116-135: 12 23 34 37 46 207 179 145 130 223
136-167: 228 227 132 133 143 135 161 201 173 106 83 91 66 53 10 9
168-203: 7 8 16 47 64 57 104 101 108 208 184 197 191 121 141 149 216 218
204-263: 152 144 134 138 199 162 176 119 158 164 174 171 170 87 169 88 107 81 82 100 98 71 59 65 50 49 26 17 13 6
264-327: 5 33 51 75 99 96 97 166 172 175 187 163 185 200 114 189 115 194 195 192 182 157 156 211 154 123 139 212 153 213 215 150
328-383: 225 224 221 220 127 147 124 193 205 206 116 160 186 167 79 85 77 92 58 62 69 54 36 32 25 18 11 4
384-455: 3 19 22 41 38 44 52 45 63 67 72 76 94 102 90 109 165 111 209 204 117 188 159 198 113 183 180 177 196 155 214 126 131 219 222 226
456-513: 230 232 262 252 418 416 413 411 376 395 283 285 379 390 363 384 388 386 361 387 360 310 354 328 315 337 349 335 324
514-561: 323 320 334 359 295 385 292 291 381 399 380 397 369 377 410 407 281 414 247 277 271 272 264 259
562-629: 237 239 244 243 275 278 250 246 417 248 394 393 370 365 300 299 364 362 298 312 313 314 353 352 343 327 350 326 319 332 333 348 347 322
630-659: 330 338 341 340 342 301 366 401 371 408 375 249 269 238 234
660-707: 257 273 255 254 245 251 412 372 282 403 396 392 391 382 389 294 297 311 344 345 318 331 325 321
708-729: 346 339 351 306 289 400 378 374 415 270 241
730-751: 231 260 268 276 409 398 290 304 308 358 316
752-765: 293 288 284 368 253 256 263
766-777: 242 274 402 383 357 329
778-789: 317 307 286 287 266 261
790-795: 236 303 356
796-803: 355 405 404 406
804-809: 235 267 302
810-815: 309 265 233
816-819: 367 296
820-837: 336 305 373 280 279 419 240 258 229
"""


def _parse_groups():
    groups, table = [], []
    for line in ROOT_GROUPS.strip().splitlines():
        span, us = line.split(":")
        first, last = (int(v) for v in span.split("-"))
        us = [int(v) for v in us.split()]
        assert first == len(table) and last - first + 1 == 2 * len(us)
        groups.append((first, last))
        for u in us:
            table += [u, NZC - u]
    return groups, table


GROUPS, ROOTS = _parse_groups()          # ROOTS[logical] = physical u
# the restricted N_CS each group of Table 5.7.2-4 is listed under: none, 15 .. 237, 237 .. 15, none
GROUP_NCS = [None] + list(NCS_RESTRICTED) + list(NCS_RESTRICTED[::-1]) + [None]

# Table 5.7.1-2 (FDD), row = config_idx % 16: (even frames only, subframes)
ROWS = {0: (True, (1,)), 1: (True, (4,)), 2: (True, (7,)), 3: (False, (1,)), 4: (False, (4,)), 5: (False, (7,)),
        6: (False, (1, 6)), 7: (False, (2, 7)), 8: (False, (3, 8)), 9: (False, (1, 4, 7)), 10: (False, (2, 5, 8)),
        11: (False, (3, 6, 9)), 12: (False, (0, 2, 4, 6, 8)), 13: (False, (1, 3, 5, 7, 9)),
        14: (False, tuple(range(10))), 15: (True, (9,))}
NA_CONFIGS = (30, 46, 60, 61, 62)


def preamble_format(config_idx):
    return -1 if config_idx > 63 or config_idx in NA_CONFIGS else config_idx // 16


def send_tti(config_idx, tti, allowed_subframe=-1):
    if preamble_format(config_idx) < 0:
        return 0
    even, sfs = ROWS[config_idx % 16]
    ok = (not even or (tti // 10) % 2 == 0) and tti % 10 in sfs
    return int(ok and allowed_subframe in (-1, tti % 10))


def d_u(u):
    p = pow(u, -1, NZC)
    return p if p < NZC / 2 else NZC - p


def restricted_params(u, N_cs):
    """(d_u, n_shift, d_start, n_group, nbar) of the restricted set, or None when the root contributes nothing"""
    d = d_u(u)
    if N_cs <= d < NZC / 3:
        n_shift = d // N_cs
        d_start = 2 * d + n_shift * N_cs
        n_group = NZC // d_start
        nbar = max((NZC - 2 * d - n_group * d_start) // N_cs, 0)
    elif NZC / 3 <= d <= (NZC - N_cs) / 2:
        n_shift = (NZC - 2 * d) // N_cs
        d_start = NZC - 2 * d + n_shift * N_cs
        n_group = d // d_start
        nbar = min(max((d - n_group * d_start) // N_cs, 0), n_shift)
    else:
        return None
    return d, n_shift, d_start, n_group, nbar


def shifts(u, N_cs, high_speed):
    """the cyclic shifts C_v of root u in increasing v"""
    if not high_speed:
        return [v * N_cs for v in range(NZC // N_cs)] if N_cs else [0]
    q = restricted_params(u, N_cs)
    if q is None:
        return []
    _, n_shift, d_start, n_group, nbar = q
    return [d_start * (v // n_shift) + (v % n_shift) * N_cs for v in range(n_shift * n_group + nbar)]


def n_cs(zero_corr_zone, high_speed):
    tab = NCS_RESTRICTED if high_speed else NCS_UNRESTRICTED
    return tab[zero_corr_zone] if zero_corr_zone < len(tab) else None


@functools.lru_cache(maxsize=None)
def cell_preambles(root_seq_idx, zero_corr_zone, high_speed):
    """([(u, C_v)] * 64, distinct roots used), or None when the configuration is invalid or gives fewer than 64"""
    N = n_cs(zero_corr_zone, high_speed)
    if N is None or root_seq_idx > 837:
        return None
    out, roots = [], 0
    for i in range(838):
        u = ROOTS[(root_seq_idx + i) % 838]
        s = shifts(u, N, high_speed)[:64 - len(out)]
        out += [(u, c) for c in s]
        roots += bool(s)
        if len(out) == 64:
            return out, roots
    return None


def resource(nof_prb, config_idx, root_seq_idx, zero_corr_zone, high_speed, freq_offset, preamble_idx):
    """the fields of mi_prach_res_t, or None for a configuration that has to be rejected"""
    f = preamble_format(config_idx)
    cell = cell_preambles(root_seq_idx, zero_corr_zone, int(bool(high_speed)))
    if nof_prb not in NFFT or f < 0 or cell is None or freq_offset > nof_prb - 6 or preamble_idx > 63:
        return None
    N_ifft = 12 * NFFT[nof_prb]
    u, C_v = cell[0][preamble_idx]
    k0 = 12 * freq_offset - 6 * nof_prb
    return dict(format=f, N_ifft=N_ifft, N_cp=CP_TS[f] * NFFT[nof_prb] // 2048, N_seq=REPS[f] * N_ifft,
                N_cs=n_cs(zero_corr_zone, high_speed), u=u, C_v=C_v, first_bin=(7 + 12 * k0 + 6) % N_ifft,
                n_roots=cell[1])


def zc(u, C_v=0):
    """x_{u,v}(n) = x_u((n + C_v) mod 839), x_u(n) = exp(-j pi u n (n + 1) / 839); the phase reduced in integers"""
    n = (np.arange(NZC) + C_v) % NZC
    return np.exp(-1j * np.pi * ((u * n * (n + 1)) % (2 * NZC)) / NZC)


def freq(u, C_v=0):
    """the preamble in frequency, unit modulus: DFT of x_{u,v} over sqrt(839)"""
    return np.fft.fft(zc(u, C_v)) / np.sqrt(NZC)


def iq(cfg, cfo=0.0, scale=1.0):
    """complex128 baseband samples (CP first) of the configuration dict cfg (the arguments of resource()): unit power
    per PRACH subcarrier, sample i multiplied by scale exp(j 2 pi cfo i / N_ul)"""
    r = resource(**cfg)
    grid = np.zeros(r["N_ifft"], complex)
    grid[(r["first_bin"] + np.arange(NZC)) % r["N_ifft"]] = freq(r["u"], r["C_v"])
    s = np.fft.ifft(grid) * np.sqrt(r["N_ifft"])
    out = np.concatenate([s[r["N_ifft"] - r["N_cp"]:]] + [s] * (r["N_seq"] // r["N_ifft"]))
    i = np.arange(len(out))
    return out * scale * np.exp(2j * np.pi * float(cfo) * i / NFFT[cfg["nof_prb"]])


def detect(sig, cfg):
    """correlation receiver for the cell of cfg on complex samples sig (the preamble delayed by less than the CP):
    drop the CP, forward FFT, the 839 PRACH bins against the conjugate DFT of every root of the cell, IDFT-839;
    the highest peak names the root, its position the cyclic-shift window and with it the preamble index; the
    delay in samples follows from the phase slope left across the bins.  Returns (preamble index, delay)."""
    r = resource(**cfg)
    cell, _ = cell_preambles(cfg["root_seq_idx"], cfg["zero_corr_zone"], int(bool(cfg["high_speed"])))
    N = r["N_ifft"]
    Y = np.fft.fft(sig[r["N_cp"]:r["N_cp"] + N])[(r["first_bin"] + np.arange(NZC)) % N] / np.sqrt(N)
    best = (0.0, None, None)
    for u in dict.fromkeys(u for u, _ in cell):
        c = np.abs(np.fft.ifft(Y * np.conj(freq(u))))
        if c.max() > best[0]:
            best = (c.max(), u, int(c.argmax()))
    _, u, peak = best
    # x_{u,v} is x_u advanced by C_v: its peak sits at lag -C_v plus the delay, inside the window of N_CS lags
    idx = None
    for i, (ui, C_v) in enumerate(cell):
        if ui == u and (r["N_cs"] == 0 or (peak + C_v) % NZC < r["N_cs"]):
            idx = i
            break
    if idx is None:
        return None, None
    z = Y * np.conj(freq(*cell[idx]))                        # exp(-j 2 pi (first_bin + k) d / N)
    slope = np.angle(np.sum(z[1:] * np.conj(z[:-1])))
    return idx, int(round(-slope * N / (2 * np.pi)))
