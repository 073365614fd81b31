"""Shapes and host arithmetic of the small-grid tests (test_small_grid_host.py,
test_gpu_small_grid.py): with the bench library's CU-count override
(fa_bench_set_cus) at K = 2 or 3, a model of 100K-500K columns is dozens of
tiles per block for every form whose grid follows the CU count.

Everything here runs without a GPU: the tile widths are read off the form
names the bench library reports, the launch geometry of the grid-stride, band
and step launchers (launch_gs, launch_gs_bands, launch_octet_bands, octet_grid,
build_step_table in csrc/fold_kernels.hpp) is restated in Python, and the
inputs are the edge-value matrices of edge_values.py plus a float16 matrix of
the classes tests/test_gpu_f16_fold.py folds.
"""
from __future__ import annotations

import functools
import re

import numpy as np

import edge_values as E

KBLOCK = 256
SEED = 2024
KS = (2, 3)                      # the pretended CU counts: an even and an odd grid
NS = (1, 2, 8, 9, 10, 17, 33)    # after the first row and for U = 2, 4, 8, 16 rows in flight: no group,
                                 # exactly one group, a group plus leftovers, two groups
NS_ALL_WIDTHS = (9, 10, 33)      # these run all three widths, the others the ragged one (index 1)
UNIT = {"f32": 4, "bf16": 8, "f16": 8, "f64": 2}  # columns per 16-byte unit
FACTOR_SETS = ("ordinary", "zero_weights")
F16 = np.float16


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ---------------------------------------------------------------------------
# tile widths, read off the form tables
# ---------------------------------------------------------------------------
def _names(B, count, name):
    return [getattr(B, name)(i).decode() for i in range(getattr(B, count)())]


def form_names(B) -> dict:
    """Every form and variant name of the bench library, by family."""
    return {
        "f32_variants": _names(B, "fa_num_variants", "fa_variant_name"),
        "f32_forms": _names(B, "fa_num_f32_forms", "fa_f32_form_name"),
        "ptrs_variants": _names(B, "fa_num_ptrs_variants", "fa_ptrs_variant_name"),
        "ptrs_forms": _names(B, "fa_num_ptrs_forms", "fa_ptrs_form_name"),
        "bf16_variants": _names(B, "fa_num_bf16_variants", "fa_bf16_variant_name"),
        "bf16_forms": _names(B, "fa_num_bf16_forms", "fa_bf16_form_name"),
        "f16_forms": _names(B, "fa_num_f16_forms", "fa_f16_form_name"),
        "rows16_forms": _names(B, "fa_num_rows16_forms", "fa_rows16_form_name"),
        "step_forms": _names(B, "fa_num_step_forms", "fa_step_form_name"),
        "step_forms_f16": _names(B, "fa_num_step_forms_f16", "fa_step_form_name_f16"),
        "step_forms_f64": _names(B, "fa_num_step_forms_f64", "fa_step_form_name_f64"),
    }


def tile_columns(name: str, unit: int) -> int:
    """The widest column tile a form's name states, 0 if it states none:
    u<rows>c<units per lane> (256 lanes, or the b<threads> / gsw<threads> the
    name gives), <n>k KiB of a row, t<units> of an LDS-staged form."""
    lanes = KBLOCK
    m = re.search(r"(?:gs\db|gsw)(\d+)_", name)
    if m:
        lanes = int(m.group(1))
    best = 0
    for m in re.finditer(r"u\d+c(\d+)", name):
        best = max(best, lanes * int(m.group(1)) * unit)
    m = re.search(r"_(\d+)k(?:_|$)", name)
    if m:
        best = max(best, int(m.group(1)) * 1024 // (16 // unit))
    m = re.search(r"_(?:w\d+)?(?:r\d+)?t(\d+)", name)
    if m:
        best = max(best, int(m.group(1)) * unit)
    return best


F64_PAIRS = (4, 2, 1)  # pick_pairs: the pair folds' pairs per lane (fa_fold_f64, fa_fedavg_f64_ptrs)


def largest_tiles(B) -> dict:
    """{element kind: T}, the largest tile in columns of any form of the family."""
    n = form_names(B)
    t32 = max(tile_columns(x, 4) for k in ("f32_variants", "f32_forms", "ptrs_variants", "ptrs_forms") for x in n[k])
    t32 = max([t32] + [tile_columns(x, 4) for x in n["step_forms"] if x.startswith("f32")])
    t16 = max(tile_columns(x, 8) for k in ("bf16_variants", "bf16_forms", "f16_forms", "rows16_forms",
                                           "step_forms_f16") for x in n[k])
    t16 = max([t16] + [tile_columns(x, 8) for x in n["step_forms"] if x.startswith("bf16")])
    t64 = max([tile_columns(x, 2) for x in n["step_forms_f64"]] + [KBLOCK * max(F64_PAIRS) * 2])
    return {"f32": t32, "bf16": t16, "f16": t16, "f64": t64}


# ---------------------------------------------------------------------------
# launch geometry, restated
# ---------------------------------------------------------------------------
def tile_grid(tiles: int, per_cu: int, cus: int) -> int:
    """octet_grid.hpp tile_grid, = launch_gs: per_cu > 0 blocks per CU, < 0 balanced passes, 0 a block per tile."""
    if tiles <= 0:
        return 0
    if per_cu == 0:
        return tiles
    g = min(abs(per_cu) * cus, tiles)
    if per_cu < 0:
        g = ceil_div(tiles, ceil_div(tiles, g))
    return g


def n_tiles(P: int, lane_units: int, unit: int, lanes: int = KBLOCK) -> int:
    units = P // unit + (1 if P % unit else 0)  # the lane of the column tail included
    return ceil_div(units, lanes * lane_units)


def bands(P: int, lane_units: int, passes: int, cus: int, unit: int):
    """launch_gs_bands / launch_octet_bands: [(first column, columns, tiles, grid)] per band launch."""
    tcols = KBLOCK * lane_units * unit
    tiles = n_tiles(P, lane_units, unit)
    nb = ceil_div(tiles, passes * cus)
    band_tiles = ceil_div(tiles, nb)
    out = []
    for b in range(nb):
        c0 = b * band_tiles * tcols
        if c0 >= P:
            break
        pb = min(P - c0, band_tiles * tcols)
        t = n_tiles(pb, lane_units, unit)
        out.append((c0, pb, t, tile_grid(t, -1, cus)))
    return out


def band_form(name: str):
    """(units per lane, passes) of a column-band form, None for any other form.
    gs_bands_16k, the fp32 policy's form, states no pass count: 3 (launch_f32_pick)."""
    m = re.search(r"bands?(\d*)_?u\d+c(\d+)", name)
    if m:
        return int(m.group(2)), int(m.group(1) or 3)
    m = re.fullmatch(r"gs_bands(\d*)_16k", name)
    if m:
        return 4, int(m.group(1) or 3)
    return None


def gs_form(name: str):
    """(lanes, units per lane, per_cu as launch_gs takes it) of a grid-stride
    form whose grid follows the CU count, None for any other form."""
    m = re.fullmatch(r"gs(\d)(?:b(\d+))?_u\d+c(\d+)nt_nts", name)  # gs1_u8c4nt_nts, gs1b512_u8c2nt_nts
    if m:
        return int(m.group(2) or KBLOCK), int(m.group(3)), int(m.group(1))
    m = re.fullmatch(r"gsbal_u\d+c(\d+)nt_nts", name)
    if m:
        return KBLOCK, int(m.group(1)), -1
    m = re.fullmatch(r"gsw(\d+)_u\d+c(\d+)", name)  # 8 one- or two-wave blocks per CU
    if m:
        return int(m.group(1)), int(m.group(2)), 8
    m = re.fullmatch(r"(?:bf16|f16_|bf16_)gs(1|bal)_?u\d+c(\d+)", name)  # bf16gs1u8c2, bf16_gsbal_u8c2, f16_gs1_u8c4
    if m:
        return KBLOCK, int(m.group(2)), 1 if m.group(1) == "1" else -1
    m = re.fullmatch(r"rows16_gsbal_u\d+c(\d+)", name)
    if m:
        return KBLOCK, int(m.group(1)), -1
    fixed = {"gs_bal_8k": (KBLOCK, 2, -1), "gs1_16k": (KBLOCK, 4, 1), "ptrs_rows_gs_16k": (KBLOCK, 4, 1)}
    return fixed.get(name)


def even_form(name: str):
    """Blocks per CU of an even-split form (k_fold_f32_even: each block walks
    its contiguous range in chunks of up to 4 quads per lane), else None."""
    m = re.fullmatch(r"even_(?:g(\d)_)?(?:auto|u\d+c\d+)", name)
    if m:
        return int(m.group(1) or 1)
    return 1 if name == "even_u4c4" else None


# Forms whose grid does not follow the CU count: they stay at one tile per
# block under the override and are run all the same (the test's docstring
# names them).  Everything else must be recognised above.
def cu_independent(name: str) -> bool:
    if name.startswith(("lds", "ring_", "qf_", "o0", "o1_", "o2_", "dw_", "pm_", "w1_", "tile_", "ptrs_o", "ptrs_dw",
                        "ptrs_lds", "bf16_tile_", "f16_tile_")):
        return True
    return name in ("u8c4nt", "u4c1nt", "xcd_u8c4nt", "v4_pickq_nts", "gsq192_u8c4nt_nts", "scalar", "column",
                    "ptrs_rows_scalar", "ptrs_generic", "rows16_column", "bf16u8c1", "bf16u8c2", "bf16u2c8")


def tiles_per_block(name: str, P: int, K: int, unit: int):
    """The most tiles one block folds in one launch of a CU-dependent form at
    K CUs (and the band count of a band form), or None: the form's grid does
    not follow the CU count, or it is a policy entry ("auto", "bf16auto") or
    "bal_u4c4nt", whose grid is the device's occupancy times the CU count."""
    bf = band_form(name)
    if bf:
        bs = bands(P, bf[0], bf[1], K, unit)
        return max(ceil_div(t, g) for _, _, t, g in bs), len(bs)
    gf = gs_form(name)
    if gf:
        t = n_tiles(P, gf[1], unit, gf[0])
        return ceil_div(t, tile_grid(t, gf[2], K)), 0
    ev = even_form(name)
    if ev:
        per = ceil_div(P // unit, ev * K)  # quads per block, in chunks of up to 4 x 256 quads
        return ceil_div(per, 4 * KBLOCK), 0
    return None


def pick_m(B, K: int) -> int:
    """Tiles of T columns in a test width: the smallest multiple of G = 2K (the
    largest CU-dependent grid the issue counts with: two blocks per CU) that
    is >= 3G and at which the 6-pass fp32 band form and every 4-pass 16-bit
    band form make at least three bands."""
    T, G, n = largest_tiles(B), 2 * K, form_names(B)
    m = 3 * G
    while True:
        ok = len(bands(m * T["f32"], 4, 6, K, 4)) >= 3
        for x in n["bf16_variants"] + n["bf16_forms"] + n["f16_forms"]:
            bf = band_form(x)
            if bf and bf[1] == 4:
                ok = ok and len(bands(m * T["bf16"], bf[0], 4, K, 8)) >= 3
        if ok:
            return m
        m += G


POLICY_F32_COLUMNS = 1 << 18  # pick_f32: below 65536 quads the fp32 policy is an LDS-staged form at any CU count


def widths(B, kind: str, K: int, policy: bool = False):
    """The three widths: on a tile boundary; a last tile of one 16-byte unit and
    a ragged tail; a last tile in which a lane has some units in range and the
    rest clamped.  Tiles are powers of two, so these place the last tile of
    every form of the family at once.  policy (fp32): m raised to the first
    multiple of G from which the fp32 shape policy leaves its LDS-staged forms
    for the tile, grid-stride and band ones (the policy entries run there)."""
    T, u, m = largest_tiles(B)[kind], UNIT[kind], pick_m(B, K)
    if policy:
        assert kind == "f32"
        m = max(m, ceil_div(ceil_div(POLICY_F32_COLUMNS, T), 2 * K) * 2 * K)
    return [m * T, m * T + u + (u - 1), m * T + KBLOCK * u + u // 2]


def cases():
    """[(K, N, width index)]: K = 2 with all three widths at N in NS_ALL_WIDTHS
    and the ragged width at the other client counts, and one run at K = 3."""
    out = [(2, N, w) for N in NS for w in range(3) if N in NS_ALL_WIDTHS or w == 1]
    return out + [(3, 10, 1)]


# ---------------------------------------------------------------------------
# inputs and expectations
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def matrix(kind: str, N: int, P: int) -> np.ndarray:
    X = {"f32": E.matrix_f32, "bf16": E.matrix_bf16, "f64": E.matrix_f64, "f16": matrix_f16}[kind](SEED, N, P)
    X.setflags(write=False)
    return X


def factor_sets(N: int, dtype):
    """The sets `ordinary` and `zero_weights` of edge_values.factor_sets, plain and scored."""
    return [(E.set_id(name, s), a, s, d) for name, a, s, d in E.factor_sets(SEED, N, dtype) if name in FACTOR_SETS]


F16_CLASSES = ("control", "all_neg_zero", "leading_neg_zero", "neg_zero_then_pos_zero", "subnormal_inputs",
               "subnormal_products", "overflow_in_order", "one_inf", "both_infs", "one_nan", "exact_cancellation",
               "random_bits", "control2")


def matrix_f16(seed: int, N: int, P: int) -> np.ndarray:
    """[N, P] float16: the edge classes of tests/test_gpu_f16_fold.py, class =
    column % 13 (as edge_values: every tile holds every class), placed by the
    row count: the special rows sit around the middle row h = N // 2."""
    K = len(F16_CLASSES)
    assert K == E.K
    rng = np.random.default_rng([seed, N, P, 400])
    X = (rng.random((N, P), dtype=np.float32) * 2 - 1).astype(F16)
    base = X.copy()
    h = N // 2

    def cols(name):
        return np.arange(F16_CLASSES.index(name), P, K)

    X[:, cols("all_neg_zero")] = F16(-0.0)
    X[:h + 1, cols("leading_neg_zero")] = F16(-0.0)
    c = cols("neg_zero_then_pos_zero")
    X[:, c] = F16(-0.0)
    X[min(h + 1, N - 1), c] = F16(0.0)
    c = cols("subnormal_inputs")
    sub = rng.integers(1, 0x400, (N, c.size)).astype(np.uint16) | (rng.integers(0, 2, (N, c.size)).astype(np.uint16) << 15)
    X[:, c] = sub.view(F16)
    c = cols("subnormal_products")
    X[:, c] = (base[:, c].astype(np.float32) * 2.0 ** -10).astype(F16)
    c = cols("overflow_in_order")
    if N >= 3:  # 60000 + 60000 = inf in client order, finite in reverse (weights permitting)
        X[h - 1, c], X[h, c], X[h + 1, c] = F16(60000), F16(60000), F16(-60000)
    c = cols("one_inf")
    X[h, c[::2]] = F16(np.inf)
    X[h, c[1::2]] = F16(-np.inf)
    c = cols("both_infs")
    X[h, c] = F16(np.inf)
    if N >= 2:
        X[h - 1, c] = F16(-np.inf)
    X[h, cols("one_nan")] = F16(np.nan)
    c = cols("exact_cancellation")
    X[:, c] = F16(-0.0)
    if N >= 2:
        X[h - 1, c] = base[h, c]
        X[h, c] = -base[h, c]
    c = cols("random_bits")
    X[:, c] = rng.integers(0, 1 << 16, (N, c.size)).astype(np.uint16).view(F16)
    return X


def f16_factor_sets(N: int):
    """[(id, weights (Python ints), scores (Python floats) or None)]: `ordinary`
    = weights 1..40, `zero_weights` = the same with the first and the last
    client at 0, as tests/test_gpu_f16_fold.py draws and zeroes them."""
    rng = np.random.default_rng([SEED, N, 401])
    w = [int(v) for v in rng.integers(1, 41, N)]
    sc = [float(v) for v in 1.0 - rng.random(N)]
    zw = list(w)
    zw[0] = zw[-1] = 0
    out = []
    for name, ws in (("ordinary", w), ("zero_weights", zw)):
        out += [(E.set_id(name, None), ws, None), (E.set_id(name, sc), ws, sc)]
    return out


def f16_divisor(w) -> float:
    """sum(w), or 1 for an all-zero draw (N <= 2), as edge_values' zero_weights."""
    return sum(w) or 1


def numpy_fold_f16(X, w, sc=None):
    """numpy's literal float16 left fold with Python-number factors (NEP 50
    keeps every operation binary16), divided by f16_divisor(w)."""
    assert all(type(v) is int for v in w) and (sc is None or all(type(v) is float for v in sc))
    with np.errstate(all="ignore"):
        acc = None
        for i in range(len(w)):
            t = X[i] * w[i] if sc is None else X[i] * w[i] * sc[i]
            acc = t if acc is None else np.add(acc, t)
        out = acc / f16_divisor(w)
    assert out.dtype == F16
    return out


def span_condition(exp: np.ndarray, T: int, all_zero_weights: bool = False) -> bool:
    """In every T-column span of the expectation there is a finite non-zero
    value and a non-finite one, so a tile cannot pass by being skipped, zeroed
    or copied from its neighbour.  The spans are the full tiles [kT, kT + T)
    and the last T columns; the partial last tile, which may be three columns
    wide, must hold a finite non-zero value (its output is NaN- or
    sentinel-filled, so skipped or zeroed it fails).  Under all-zero weights
    (`zero_weights` at N <= 2, where that set zeroes the first and the last
    client) every result is 0 * x: no finite non-zero value can exist, and a
    finite zero stands in for it."""
    e = np.asarray(exp)
    if e.dtype == np.uint16:
        raise TypeError("pass values, not bit patterns")
    e = e.astype(np.float64) if e.dtype != np.float64 else e
    fin = np.isfinite(e)
    want = fin & (e == 0) if all_zero_weights else fin & (e != 0)
    full = e.size // T * T
    for lo in list(range(0, full, T)) + [e.size - T]:
        if not want[lo:lo + T].any() or fin[lo:lo + T].all():
            return False
    return full == e.size or bool(want[full:].any())


# ---------------------------------------------------------------------------
# the one-launch step: its table and its schedule, restated
# ---------------------------------------------------------------------------
# name -> (wide units per lane, narrow units per lane, pool100, last_only, round_tail, bal): kStepSpecs*
STEP_SPECS = {
    "bf16_step_bal_u8c4": (4, 2, 0, True, False, True),
    "f32_step_sd_u8c4_p75": (4, 1, 75, False, False, False),
    "bf16_step_rt_u8c4n8c2_p100_last": (4, 2, 100, True, True, False),
    "bf16_step_static_u8c4": (4, 4, 0, False, False, False),
    "f32_step_bal_u8c4": (4, 1, 0, True, False, True),
    "f16_step_bal_u8c4": (4, 2, 0, True, False, True),
    "f16_step_static_u8c4": (4, 4, 0, False, False, False),
    "f64_step_bal_u8c4": (4, 2, 0, True, False, True),
    "f64_step_sd_u8c4_p75": (4, 1, 75, False, False, False),
    "f64_step_static_u8c4": (4, 4, 0, False, False, False),
}


def step_unit(name: str) -> int:
    return 8 if name.startswith(("bf16", "f16")) else 2 if name.startswith("f64") else 4


def step_table(name: str, offsets, grid: int):
    """build_step_table: [dict(col0, width, round, small, tiles, stride, static)] in the launch's tile order."""
    cb, cs, pool100, last_only, round_tail, bal = STEP_SPECS[name]
    ucols, rounds = step_unit(name), len(offsets) - 1
    wide = KBLOCK * cb * ucols
    pool = pool100 * grid * wide // 100
    if last_only:
        pool = min(pool, offsets[-1] - offsets[-2])
    split = [0] * rounds
    for k in range(rounds - 1, -1, -1):
        w = offsets[k + 1] - offsets[k]
        assert w >= 1 and offsets[k] % ucols == 0
        if pool <= 0:
            split[k] = w
        elif pool >= w:
            split[k], pool = 0, pool - w
        else:
            split[k], pool = (w - pool) // wide * wide, 0
    segs = []

    def add(k, lo, hi, small, static):
        per = KBLOCK * (cs if small else cb)
        n = ceil_div(ceil_div(hi - lo, ucols), per)
        segs.append(dict(col0=offsets[k] + lo, width=hi - lo, round=k, small=small, tiles=n, per=per * ucols,
                         stride=ceil_div(n, ceil_div(n, grid)), static=static))

    for p in (0, 1):
        for k in range(rounds):
            w = offsets[k + 1] - offsets[k]
            lo, hi = (0, split[k]) if p == 0 else (split[k], w)
            if hi <= lo:
                continue
            if p == 0 and round_tail and not bal and k + 1 < rounds:
                mid = lo + (hi - lo) // wide // grid * grid * wide
                if mid > lo:
                    add(k, lo, mid, False, True)
                if hi > mid:
                    add(k, mid, hi, True, True)
                continue
            add(k, lo, hi, p == 1, p == 0)
    return segs


def step_coverage(name: str, offsets, K: int):
    """How often the launch of step form `name` on K blocks folds each column
    of [0, offsets[-1]) (it must be exactly once), and the most wide tiles of
    one round that one block holds.  Static tiles are dealt as step_tiles
    (tile t to block t % grid) or step_tiles_bal (tile i of a segment to block
    i % stride, stride <= grid) deal them; a pool tile goes to any block."""
    segs = step_table(name, offsets, K)
    total = sum(s["tiles"] for s in segs)
    grid = min(K, total)
    bal = STEP_SPECS[name][5]
    count = np.zeros(offsets[-1], np.int32)
    held = {}
    t0 = 0
    for s in segs:
        assert not s["static"] or not bal or 1 <= s["stride"] <= grid, (name, s)
        for i in range(s["tiles"]):
            lo = s["col0"] + i * s["per"]
            hi = min(lo + s["per"], s["col0"] + s["width"])
            assert lo < hi, (name, s, i)
            count[lo:hi] += 1
            if s["static"] and not s["small"]:
                b = i % s["stride"] if bal else (t0 + i) % grid
                held[(s["round"], b)] = held.get((s["round"], b), 0) + 1
        t0 += s["tiles"]
    return count, (max(held.values()) if held else 0)


def step_offsets(kind: str, P: int, align: int = 64):
    """Three rounds over [0, P): every start a multiple of the slot alignment
    (sharding.ALIGN), the last round ragged (it ends at P)."""
    q = P // 4 // align * align
    return [0, q, 3 * q, P]
