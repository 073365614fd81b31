"""Every grid-stride, band and step form at several tiles per block.

Every launch geometry follows cu_count(): on a 256-CU device a block folds a
second tile only from about a million columns on, so the rest of the suite
walks a block from one tile to the next at a handful of shapes, none of them
with edge values, a clamped last tile or a continued accumulator.  Here the
bench library's override (fa_bench_set_cus) pretends K = 2 CUs (one run: K = 3,
an odd grid), and every form of every family folds the edge-value matrices of
tests/edge_values.py at 100K-500K columns, bit for bit against the C oracle
(float16: numpy's float16 left fold, on the classes of
tests/test_gpu_f16_fold.py).  NaN is compared by position, everything else by
its bits; the bf16 bits also against an independent rounding.

Shapes (tests/small_grid.py; tests/test_small_grid_host.py checks all of this
without a GPU).  T = the largest tile in columns of any form of the family, read
off the form names: 8192 fp32, 16384 16-bit, 2048 float64 columns.  G = 2K, m =
the smallest multiple of G that is >= 3G and gives the 6-pass fp32 band form
and the 4-pass 16-bit band forms three bands.  Widths: m*T (ends on a tile
boundary), m*T + unit + (unit - 1) (a last tile of one 16-byte unit and a ragged
tail), m*T + 256*unit + unit/2 (a last tile in which a lane has some units in
range and the rest clamped); tiles are powers of two, so every form's last tile
is placed at once.  P // T >= 3G is asserted, and with it at least three tiles
in some block of every form whose grid follows the CU count (a band form: its
pass count per band launch, two for the 2-pass forms, and the band count the
restated arithmetic of launch_gs_bands / launch_octet_bands gives).

Client counts 1, 2, 8, 9, 10, 17, 33: after the first row no group of U = 2, 4,
8 or 16 rows in flight, exactly one, one and leftover rows, two.  All three
widths run at N = 9, 10 and 33, the ragged width alone at the other counts
(the full matrix would triple the file's time for the same tile walks), and
K = 3 at N = 10 on the ragged width.  Factor sets `ordinary` and `zero_weights`,
plain and scored.  Before any launch: every T-column span of every expectation
holds a finite non-zero and a non-finite value (small_grid.span_condition; under
the all-zero weights that `zero_weights` is at N <= 2, a zero and a NaN), so a
tile cannot pass skipped, zeroed or copied from its neighbour.  Outputs are
NaN- or sentinel-filled with a guard region behind them that must stay as it
was.

Forms whose grid does not follow the CU count stay at one tile per block and
run all the same: the one-block-per-tile forms (u8c4nt, u4c1nt, xcd_u8c4nt,
v4_pickq_nts, tile_*, bf16u8c1 / u8c2 / u2c8, bf16_tile_*, f16_tile_*), the
LDS-staged, ring and one-wave forms (lds*, ring_*, qf_*, o0* / o1_* / o2_*,
dw_*, pm_*, w1_*, ptrs_o*, ptrs_dw_*, ptrs_lds_*: one block per t<quads> tile),
the one-column-per-lane forms (scalar, column, ptrs_rows_scalar, ptrs_generic,
rows16_column) and gsq192_u8c4nt_nts, a fixed 192 blocks, more than these
widths have tiles.  bal_u4c4nt sizes its grid by the device's occupancy times
the CU count: several chunks per block, how many is the device's to say.  The
layer-table folds are left out: their grid_cap already does this
(tests/test_gpu_layers.py).
"""
import ctypes
import functools

import numpy as np
import pytest

import edge_values as E
import small_grid as SG
from oracle import oracle_lib as OL  # checker

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT16 = 0x5A5A  # a 16-bit output element no kernel writes keeps this pattern
F16 = np.float16
CASES = SG.cases()
IDS = ["K%d-N%d-w%d" % c for c in CASES]
NS_PICK = [1, 10, 48, 100, 300, 1024]
PS_PICK = [40000, 300_003, 582_000, 1_000_000, 2_100_003, 25_000_000]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def libs():
    from fedlesscan_amd import _lib
    B = _lib.load_bench()
    yield _lib, _lib.load(), B
    assert B.fa_bench_set_cus(0) == 0, "the CU-count override outlived the module"


def _picks(B, cus):
    return [B.fa_f32_pick_name(N, P, cus) for N in NS_PICK for P in PS_PICK]


@pytest.fixture()
def grid(request, libs):
    """(K, N, width index) with the override at K; proves that the library sees it."""
    _lib, L, B = libs
    K, N, w = request.param
    real = _picks(B, 0)
    assert B.fa_bench_set_cus(K) == 0
    try:
        seen = _picks(B, 0)
        assert seen == _picks(B, K) and seen != real, "the override does not reach cu_count()"
        yield K, N, w
    finally:
        torch.cuda.synchronize()
        assert B.fa_bench_set_cus(0) == K


both = pytest.mark.parametrize("grid", CASES, ids=IDS, indirect=True)


# ---------------------------------------------------------------------------
# inputs and expectations: once per (kind, N, P), shared, never modified
# ---------------------------------------------------------------------------
def _T(B, kind):
    return SG.largest_tiles(B)[kind]


@functools.lru_cache(maxsize=8)
def _cases(kind, N, P, T):
    """[(id, a, s or None, divisor, expected)], each expectation checked for the span condition."""
    X = SG.matrix(kind, N, P)
    out = []
    if kind == "f16":
        for fid, w, sc in SG.f16_factor_sets(N):
            exp = SG.numpy_fold_f16(X, w, sc)
            assert SG.span_condition(exp, T, not any(w)), (kind, N, P, fid)
            with np.errstate(all="ignore"):
                a = np.array([F16(v) for v in w], F16)
                s = None if sc is None else np.array([F16(v) for v in sc], F16)
                d = F16(SG.f16_divisor(w))
            out.append((fid, a, s, d, exp))
        return out
    for fid, a, s, d in SG.factor_sets(N, np.float64 if kind == "f64" else np.float32):
        if kind == "f32":
            exp = OL.fedavg_f32(X, a, d, s=s)
        elif kind == "f64":
            exp = OL.fedavg_f64(X, a, d, s=s)
        else:
            exp = OL.fedavg_bf16(X, a, d, s=s)
            # the oracle's bf16 bits against a rounding that does not share its expression: the
            # outputs below are held to these bits, so they are held to the independent rounding
            assert E.bf16_matches_independent(exp[1], exp[0]), (N, P, fid)
        assert SG.span_condition(exp[0] if kind == "bf16" else exp, T, not a.any()), (kind, N, P, fid)
        out.append((fid, a, s, d, exp))
    assert len(out) == 2 * len(SG.FACTOR_SETS)
    return out


def _shape(libs, grid, kind):
    _lib, L, B = libs
    K, N, w = grid
    T, P = _T(B, kind), SG.widths(B, kind, K)[w]
    assert P // T >= 3 * 2 * K
    return K, N, P, T


def _assert_tiles_per_block(names, P, K, unit):
    """At least three tiles in some block of every form whose grid follows the
    CU count (a band form: its passes per band launch), and the band counts."""
    n = 0
    for x in names:
        tb = SG.tiles_per_block(x, P, K, unit)
        if tb is None:
            assert x in ("auto", "bf16auto", "bal_u4c4nt") or SG.cu_independent(x), x
            continue
        n += 1
        bf = SG.band_form(x)
        assert tb[0] >= (3 if bf is None else min(3, bf[1])), (x, P, tb)
        if bf is not None:
            assert tb[1] == len(SG.bands(P, bf[0], bf[1], K, unit)) >= 2, (x, P, tb)
            assert tb[1] >= 3 or not (bf[1] == 4 or (unit == 4 and bf[1] == 6)), (x, P, tb)
    return n


def _dev_bits(x, dev):
    """A numpy array on the device, 16-bit types through their bit patterns (int16)."""
    x = np.ascontiguousarray(x)
    if x.dtype in (np.uint16, np.float16):
        x = x.view(np.int16)
    return torch.from_numpy(x.copy()).to(dev)


def _factors(dev, a, s):
    ad = _dev_bits(a, dev)
    sd = None if s is None else _dev_bits(s, dev)
    return ad, sd, (None if sd is None else sd.data_ptr())


def _half_bits(d) -> int:
    return int(np.asarray(d, F16).view(np.uint16))


def _stacked(dev, Xh, ldx, off=0):
    """The rows of Xh at pitch ldx, the first at element `off` of a buffer whose
    every other element is NaN.  Returns (buffer, [N, P] view)."""
    N, P = Xh.shape
    if Xh.dtype.itemsize == 2:
        nan16 = 0x7FC0 if Xh.dtype == np.uint16 else 0x7E00
        buf = torch.full((N * ldx + off + 8,), nan16, dtype=torch.int16, device=dev)
    else:
        buf = torch.full((N * ldx + off + 8,), float("nan"),
                         dtype=torch.float64 if Xh.dtype == np.float64 else torch.float32, device=dev)
    view = buf[off:off + N * ldx].view(N, ldx)[:, :P]
    view.copy_(_dev_bits(Xh, dev))
    return buf, view


def _separate_rows(dev, Xh, shift=0):
    """Each row its own allocation; shift = 1: every row one element past a 16-B boundary."""
    rows, keep = [], []
    for i in range(Xh.shape[0]):
        src = _dev_bits(Xh[i], dev)
        holder = torch.zeros(src.numel() + shift, dtype=src.dtype, device=dev)
        holder[shift:].copy_(src)
        keep.append(holder)
        rows.append(holder[shift:])
    assert all((r.data_ptr() % 16 == 0) == (shift == 0) for r in rows)
    return rows, torch.tensor([r.data_ptr() for r in rows], dtype=torch.int64, device=dev), keep


def _outs(dev, n, P, dtype=torch.float32):
    """n output rows of P elements, 16-B aligned, NaN-filled (16-bit: the
    sentinel), each with a guard of at least 16 bytes behind it."""
    per = 16 // torch.empty(0, dtype=dtype).element_size()
    w = (P + per - 1) // per * per + per
    return torch.full((n, w), SENT16 if dtype == torch.int16 else float("nan"), dtype=dtype, device=dev)


_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def _nan(t, nan16):
    return ((t & 0x7FFF) > nan16) if t.dtype == torch.int16 else torch.isnan(t)


def _check(o, names, exp, P, what, nan16=None, shift=0):
    """Rows of o (launched into _outs rows at element `shift`) against exp on the
    device: NaN by position, every other element by its bits, and nothing
    written before or behind.  nan16: the largest non-NaN magnitude pattern
    of a 16-bit format (0x7F80 bf16, 0x7C00 float16)."""
    assert o.shape[0] == len(names)
    e = _dev_bits(exp, o.device)
    got = o[:, shift:shift + P]
    gb, eb = got.view(_INT[got.element_size()]), e.view(_INT[e.element_size()])
    ok = (gb == eb[None]) | (_nan(got, nan16) & _nan(e, nan16)[None])
    rows = ok.all(dim=1).cpu().numpy()
    if not rows.all():
        k = int(np.flatnonzero(~rows)[0])
        cols = np.flatnonzero(~ok[k].cpu().numpy())
        raise AssertionError((what, "wrong:", [names[i] for i in np.flatnonzero(~rows)], "first:", names[k],
                              "%d columns, from %d" % (cols.size, cols[0]), "got", hex(int(gb[k, cols[0]])),
                              "expected", hex(int(eb[cols[0]]))))
    guard = torch.cat([o[:, :shift], o[:, shift + P:]], dim=1)
    untouched = (guard == SENT16) if o.dtype == torch.int16 else torch.isnan(guard)
    assert bool(untouched.all()), (what, "wrote outside out", [names[i] for i in
                                                              np.flatnonzero(~untouched.all(dim=1).cpu().numpy())])


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------------------
# fp32 stacked
# ---------------------------------------------------------------------------
@both
def test_f32_every_variant_and_form(dev, libs, grid):
    """Every fa_fedavg_f32_variant (0: the policy, which under the override
    picks its grid-stride and band branches) and every fa_fedavg_f32_form."""
    _lib, L, B = libs
    K, N, P, T = _shape(libs, grid, "f32")
    vnames = [B.fa_variant_name(v).decode() for v in range(B.fa_num_variants())]
    fnames = [B.fa_f32_form_name(f).decode() for f in range(B.fa_num_f32_forms())]
    assert _assert_tiles_per_block(vnames + fnames, P, K, 4) >= 20
    names = vnames + ["form " + x for x in fnames]
    ldx = (P + 3) // 4 * 4 + 4
    buf, X = _stacked(dev, SG.matrix("f32", N, P), ldx)
    st = _stream(dev)
    for fid, a, s, d, exp in _cases("f32", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        o = _outs(dev, len(names), P)
        for v in range(len(vnames)):
            _lib.check(B.fa_fedavg_f32_variant(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, float(d), o[v].data_ptr(),
                                               st, v), vnames[v], bench=True)
        for f in range(len(fnames)):
            _lib.check(B.fa_fedavg_f32_form(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, float(d),
                                            o[len(vnames) + f].data_ptr(), st, f), fnames[f], bench=True)
        _check(o, names, exp, P, (fid, K, N, P))


@both
def test_f32_policy_at_its_large_model_branches(dev, libs, grid):
    """Variant 0 once more, where the fp32 policy has left its LDS-staged forms
    (below 65536 quads it picks one at any CU count, so at the widths above
    variant 0 is one block per tile): the band form at 24 clients and more,
    one block per 16 KiB tile below."""
    _lib, L, B = libs
    K, N, w = grid
    T = _T(B, "f32")
    P = SG.widths(B, "f32", K, policy=True)[w]
    pick = B.fa_f32_pick_name(N, P, 0).decode()
    assert pick == ("gs_bands_16k" if N >= 24 else "tile_16k"), pick
    assert N < 24 or SG.tiles_per_block(pick, P, K, 4)[1] >= 3
    ldx = (P + 3) // 4 * 4 + 4
    buf, X = _stacked(dev, SG.matrix("f32", N, P), ldx)
    st = _stream(dev)
    for fid, a, s, d, exp in _cases("f32", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        o = _outs(dev, 1, P)
        _lib.check(B.fa_fedavg_f32_variant(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, float(d), o[0].data_ptr(), st,
                                           0), "auto", bench=True)
        _check(o, ["auto (" + pick + ")"], exp, P, (fid, K, N, P))


@both
def test_f32_row_tables(dev, libs, grid):
    """Every fa_fedavg_f32_ptrs_variant and fa_fedavg_f32_ptrs_form on 16-B
    aligned rows; the any-alignment variants also on rows at a 4-byte offset,
    into an output at a 4-byte offset."""
    _lib, L, B = libs
    K, N, P, T = _shape(libs, grid, "f32")
    Xh = SG.matrix("f32", N, P)
    rows, tab, _k1 = _separate_rows(dev, Xh)
    rows_o, tab_o, _k2 = _separate_rows(dev, Xh, shift=1)
    vnames = [B.fa_ptrs_variant_name(v).decode() for v in range(B.fa_num_ptrs_variants())]
    fnames = [B.fa_ptrs_form_name(f).decode() for f in range(B.fa_num_ptrs_forms())]
    assert _assert_tiles_per_block(fnames, P, K, 4) >= 1  # ptrs_rows_gs_16k
    anyal = [v for v in range(len(vnames)) if vnames[v].startswith(("ptrs_dw", "ptrs_rows_scalar", "ptrs_generic"))]
    assert len(anyal) >= 6
    names = vnames + ["form " + x for x in fnames]
    onames = [vnames[v] + " rows at 4 B" for v in anyal]
    st = _stream(dev)
    for fid, a, s, d, exp in _cases("f32", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        o, oo = _outs(dev, len(names), P), _outs(dev, len(onames), P + 1)
        for v in range(len(vnames)):
            _lib.check(B.fa_fedavg_f32_ptrs_variant(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d),
                                                    o[v].data_ptr(), st, v), vnames[v], bench=True)
        for f in range(len(fnames)):
            _lib.check(B.fa_fedavg_f32_ptrs_form(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d),
                                                 o[len(vnames) + f].data_ptr(), st, f), fnames[f], bench=True)
        for k, v in enumerate(anyal):
            _lib.check(B.fa_fedavg_f32_ptrs_variant(tab_o.data_ptr(), N, P, ad.data_ptr(), sp, float(d),
                                                    oo[k, 1:].data_ptr(), st, v), onames[k], bench=True)
        _check(o, names, exp, P, (fid, K, N, P))
        _check(oo, onames, exp, P, (fid, K, N, P), shift=1)


# ---------------------------------------------------------------------------
# bf16 and float16 stacked, the 16-bit row tables
# ---------------------------------------------------------------------------
@both
def test_bf16_every_variant_and_form(dev, libs, grid):
    """Every fa_fedavg_bf16_variant (0: the policy) and fa_fedavg_bf16_form,
    with both outputs and with the bf16 output alone."""
    _lib, L, B = libs
    K, N, P, T = _shape(libs, grid, "bf16")
    vnames = [B.fa_bf16_variant_name(v).decode() for v in range(B.fa_num_bf16_variants())]
    fnames = [B.fa_bf16_form_name(f).decode() for f in range(B.fa_num_bf16_forms())]
    assert _assert_tiles_per_block(vnames + fnames, P, K, 8) >= 19
    names = vnames + ["form " + x for x in fnames]
    n = len(names)
    ldx = (P + 7) // 8 * 8 + 8
    buf, X = _stacked(dev, SG.matrix("bf16", N, P), ldx)
    st = _stream(dev)

    def launch(k, ad, sp, d, of, ob):
        if k < len(vnames):
            rc = B.fa_fedavg_bf16_variant(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, d, of, ob, st, k)
        else:
            rc = B.fa_fedavg_bf16_form(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, d, of, ob, st, k - len(vnames))
        _lib.check(rc, names[k], bench=True)

    for fid, a, s, d, (ef, eb) in _cases("bf16", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        of, ob, ob1 = _outs(dev, n, P), _outs(dev, n, P, torch.int16), _outs(dev, n, P, torch.int16)
        for k in range(n):
            launch(k, ad, sp, float(d), of[k].data_ptr(), ob[k].data_ptr())
            launch(k, ad, sp, float(d), None, ob1[k].data_ptr())
        _check(of, names, ef, P, (fid, K, N, P, "fp32 out"))
        _check(ob, names, eb, P, (fid, K, N, P, "bf16 out"), nan16=0x7F80)
        _check(ob1, names, eb, P, (fid, K, N, P, "bf16 out alone"), nan16=0x7F80)


@both
def test_f16_every_form(dev, libs, grid):
    """Every fa_fedavg_f16_form against numpy's float16 left fold."""
    _lib, L, B = libs
    K, N, P, T = _shape(libs, grid, "f16")
    names = [B.fa_f16_form_name(f).decode() for f in range(B.fa_num_f16_forms())]
    assert _assert_tiles_per_block(names, P, K, 8) >= 7
    ldx = (P + 7) // 8 * 8 + 8
    buf, X = _stacked(dev, SG.matrix("f16", N, P), ldx)
    st = _stream(dev)
    for fid, a, s, d, exp in _cases("f16", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        o = _outs(dev, len(names), P, torch.int16)
        for f in range(len(names)):
            _lib.check(B.fa_fedavg_f16_form(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, _half_bits(d), o[f].data_ptr(),
                                            st, f), names[f], bench=True)
        _check(o, names, exp, P, (fid, K, N, P), nan16=0x7C00)


@both
def test_16_bit_row_tables(dev, libs, grid):
    """Every fa_fedavg_bf16_ptrs_form (both outputs, and the bf16 one alone)
    and fa_fedavg_f16_ptrs_form on 16-B aligned rows, the policy (-1) included;
    the column form also with the rows not promised aligned."""
    _lib, L, B = libs
    K, N, P, T = _shape(libs, grid, "bf16")
    fnames = [B.fa_rows16_form_name(f).decode() for f in range(B.fa_num_rows16_forms())]
    assert _assert_tiles_per_block(fnames, P, K, 8) >= 4
    runs = [(x, f, 1) for f, x in enumerate(fnames)] + [("policy aligned", -1, 1), ("policy", -1, 0)]
    runs += [(x + " unpromised", f, 0) for f, x in enumerate(fnames) if x.endswith("column")]
    assert len(runs) == len(fnames) + 3
    names = [r[0] for r in runs]
    n = len(runs)
    st = _stream(dev)
    rows, tab, _k1 = _separate_rows(dev, SG.matrix("bf16", N, P))
    for fid, a, s, d, (ef, eb) in _cases("bf16", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        of, ob, ob1 = _outs(dev, n, P), _outs(dev, n, P, torch.int16), _outs(dev, n, P, torch.int16)
        for k, (name, f, al) in enumerate(runs):
            _lib.check(B.fa_fedavg_bf16_ptrs_form(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), al,
                                                  of[k].data_ptr(), ob[k].data_ptr(), st, f), name, bench=True)
            _lib.check(B.fa_fedavg_bf16_ptrs_form(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), al, None,
                                                  ob1[k].data_ptr(), st, f), name + " bf16 only", bench=True)
        _check(of, names, ef, P, (fid, K, N, P, "fp32 out"))
        _check(ob, names, eb, P, (fid, K, N, P, "bf16 out"), nan16=0x7F80)
        _check(ob1, names, eb, P, (fid, K, N, P, "bf16 out alone"), nan16=0x7F80)
    del rows, tab, _k1
    rows, tab, _k1 = _separate_rows(dev, SG.matrix("f16", N, P))
    for fid, a, s, d, exp in _cases("f16", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        o = _outs(dev, n, P, torch.int16)
        for k, (name, f, al) in enumerate(runs):
            _lib.check(B.fa_fedavg_f16_ptrs_form(tab.data_ptr(), N, P, ad.data_ptr(), sp, _half_bits(d), al,
                                                 o[k].data_ptr(), st, f), "f16 " + name, bench=True)
        _check(o, names, exp, P, (fid, K, N, P, "float16"), nan16=0x7C00)


# ---------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------
@both
def test_f64_fold_and_row_table(dev, libs, grid):
    """fa_bench_fold_f64 as a one-shot fold on 16-B aligned rows of an even pitch
    (the pair kernel) and through a view at an 8-byte offset with an odd pitch
    (one column per lane); fa_bench_fedavg_f64_ptrs with the rows promised
    aligned (the pair kernel) and not."""
    _lib, L, B = libs
    K, N, P, T = _shape(libs, grid, "f64")
    assert SG.ceil_div(SG.n_tiles(P, max(SG.F64_PAIRS), 2), K) >= 3  # the balanced grid is at most K blocks
    Xh = SG.matrix("f64", N, P)
    ldx = (P + 1) // 2 * 2 + 2
    _b1, Xv = _stacked(dev, Xh, ldx)
    _b2, Xo = _stacked(dev, Xh, ldx + 1, off=1)
    assert Xv.data_ptr() % 16 == 0 and Xo.data_ptr() % 16 == 8
    rows, tab, _k1 = _separate_rows(dev, Xh)
    st = _stream(dev)
    names = ["fold pairs", "fold one column per lane", "row table pairs", "row table one column per lane"]
    for fid, a, s, d, exp in _cases("f64", N, P, T):
        ad, sd, sp = _factors(dev, a, s)
        o = _outs(dev, 4, P, torch.float64)
        _lib.check(B.fa_bench_fold_f64(Xv.data_ptr(), N, P, ldx, ad.data_ptr(), sp, None, float(d), 1, o[0].data_ptr(),
                                       st), names[0], bench=True)
        _lib.check(B.fa_bench_fold_f64(Xo.data_ptr(), N, P, ldx + 1, ad.data_ptr(), sp, None, float(d), 1,
                                       o[1].data_ptr(), st), names[1], bench=True)
        _lib.check(B.fa_bench_fedavg_f64_ptrs(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), 1, o[2].data_ptr(),
                                              st), names[2], bench=True)
        _lib.check(B.fa_bench_fedavg_f64_ptrs(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), 0, o[3].data_ptr(),
                                              st), names[3], bench=True)
        _check(o, names, exp, P, (fid, K, N, P))


@pytest.mark.parametrize("d", [2.0, 6.0, 1000.0, 3168.0, -3168.0])
def test_f64_subnormal_quotients_on_and_beside_a_tie(dev, libs, d):
    """What the shapes above found at 10 x 40963, column 9948: -49104 x 2^-1074 /
    3168 = -15.5 x 2^-1074 is a tie, and IEEE 754 (and numpy) round it to the
    even -16 x 2^-1074.  Here every column's sum is (2n + 1) x d/2 units of
    2^-1074 (a tie for every n), or one unit beside it, split over two clients
    whose add is exact; n reaches up to the last subnormal.  No override: the
    product's fa_fedavg_f64 kernels and the pair folds, against numpy's divide."""
    _lib, L, B = libs
    P = 4099
    rng = np.random.default_rng([SG.SEED, 500])
    top = (1 << 52) - 1 if abs(d) == 2.0 else (1 << 30)
    n = np.concatenate([np.arange(64), rng.integers(0, top, P - 128), top - 1 - np.arange(64)]).astype(np.int64)
    beside = rng.integers(-1, 2, P)  # on the tie, or one unit beside it
    units = (2 * n + 1) * int(abs(d) / 2) + beside
    assert (units < (1 << 53)).all() and (beside == 0).sum() > 1000
    first = rng.integers(0, 1 << 20, P) % (units + 1)
    sign = np.where(rng.integers(0, 2, P) == 1, -1.0, 1.0)
    Xh = np.stack([first, units - first]).astype(np.float64) * 2.0 ** -1074 * sign
    a = np.ones(2)
    with np.errstate(all="ignore"):
        exp = np.true_divide(Xh[0] * a[0] + Xh[1] * a[1], np.float64(d))
    assert (np.abs(exp) < 2.0 ** -1022).sum() >= P - 64 and (exp != 0).sum() >= P - 64
    ldx = P + 4  # odd, and ldx - 1 even: the pair kernels' pitch
    _b1, Xv = _stacked(dev, Xh, ldx - 1)
    _b2, Xo = _stacked(dev, Xh, ldx, off=1)
    assert Xv.data_ptr() % 16 == 0 and (ldx - 1) % 2 == 0 and Xo.data_ptr() % 16 == 8
    rows, tab, _k1 = _separate_rows(dev, Xh)
    ad, sd, sp = _factors(dev, a, None)
    st = _stream(dev)
    names = ["fa_fedavg_f64 pairs", "fa_fedavg_f64 one column per lane", "fold pairs", "fold one column per lane",
             "row table pairs", "row table one column per lane"]
    o = _outs(dev, len(names), P, torch.float64)
    _lib.check(L.fa_fedavg_f64(Xv.data_ptr(), 2, P, ldx - 1, ad.data_ptr(), None, d, o[0].data_ptr(), st), names[0])
    _lib.check(L.fa_fedavg_f64(Xo.data_ptr(), 2, P, ldx, ad.data_ptr(), None, d, o[1].data_ptr(), st), names[1])
    _lib.check(B.fa_bench_fold_f64(Xv.data_ptr(), 2, P, ldx - 1, ad.data_ptr(), None, None, d, 1, o[2].data_ptr(), st),
               names[2], bench=True)
    _lib.check(B.fa_bench_fold_f64(Xo.data_ptr(), 2, P, ldx, ad.data_ptr(), None, None, d, 1, o[3].data_ptr(), st),
               names[3], bench=True)
    for k, al in ((4, 1), (5, 0)):
        _lib.check(B.fa_bench_fedavg_f64_ptrs(tab.data_ptr(), 2, P, ad.data_ptr(), None, d, al, o[k].data_ptr(), st),
                   names[k], bench=True)
    _check(o, names, exp, P, ("ties", d))


# ---------------------------------------------------------------------------
# chunked folds: the accumulator carried in place from tile to tile and cut to cut
# ---------------------------------------------------------------------------
@both
def test_chunked_folds_in_place(dev, libs, grid):
    """fa_bench_fold_f32 / _f16 / _f64 in three cuts ({0, 1, (N + 1) // 2, N}),
    acc_in == out, only the last cut dividing: the vector layout of each, and
    fp32 also on an odd pitch at a 4-byte offset.  The float16 and float64
    folds are grid-stride at any row count.  The fp32 fold takes the policy's
    form for each cut's own row count: the vector layout runs at the widths
    where that is one block per 16 KiB tile below 24 rows and the band form
    from 24 on, and at N >= 26 three more cut sets give the band form a first
    cut, a continuing middle cut and a dividing last cut of 24 rows or more."""
    _lib, L, B = libs
    K, N, w = grid
    st = _stream(dev)
    base = sorted({0, min(1, N), (N + 1) // 2, N})
    runs = [("f32", "vector", B.fa_bench_fold_f32), ("f32", "odd_pitch", B.fa_bench_fold_f32),
            ("f16", "vector", B.fa_bench_fold_f16), ("f64", "vector", B.fa_bench_fold_f64)]
    for kind, layout, fold in runs:
        _, _, P, T = _shape(libs, grid, kind)
        u = SG.UNIT[kind]
        cut_sets = [base]
        if kind == "f32" and layout == "vector":
            P = SG.widths(B, "f32", K, policy=True)[w]
            if N >= 26:
                cut_sets += [[0, 1, 25, N], [0, 1, N], [0, 25, N]]
            picks = {(c > 0, r1 == N): B.fa_f32_pick_name(r1 - r0, P, 0).decode()
                     for cs_ in cut_sets[1:] for c, (r0, r1) in enumerate(zip(cs_[:-1], cs_[1:])) if r1 - r0 >= 24}
            assert N < 26 or (len(picks) == 3 and set(picks.values()) == {"gs_bands_16k"}), picks
            assert all(B.fa_f32_pick_name(r1 - r0, P, 0) == b"tile_16k" for r0, r1 in zip(base[:-1], base[1:]))
        if layout == "vector":
            ldx, off = (P + u - 1) // u * u + u, 0
        else:
            ldx, off = (P + 2 if P % 2 else P + 1), 1
        buf, X = _stacked(dev, SG.matrix(kind, N, P), ldx, off)
        assert (X.data_ptr() % 16 == 0) == (layout == "vector")
        cs = _cases(kind, N, P, T)
        dt = {"f32": torch.float32, "f16": torch.int16, "f64": torch.float64}[kind]
        o = _outs(dev, len(cs) * len(cut_sets), P + 1, dt)
        for k, (fid, a, s, d, exp) in enumerate(cs):
            ad, sd, sp = _factors(dev, a, s)
            esz = ad.element_size()
            for j, cuts in enumerate(cut_sets):
                acc = o[k * len(cut_sets) + j, off:]
                for c, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
                    _lib.check(fold(X[r0].data_ptr(), r1 - r0, P, ldx, ad.data_ptr() + r0 * esz,
                                    None if sp is None else sp + r0 * esz, None if c == 0 else acc.data_ptr(),
                                    _half_bits(d) if kind == "f16" else float(d), int(r1 == N), acc.data_ptr(), st),
                               "fold " + kind, bench=True)
        for k, (fid, a, s, d, exp) in enumerate(cs):
            _check(o[k * len(cut_sets):(k + 1) * len(cut_sets)], ["fold %s %s %s" % (kind, layout, c) for c in cut_sets],
                   exp, P, (fid, K, N, P), shift=off, nan16=0x7C00 if kind == "f16" else None)


# ---------------------------------------------------------------------------
# the one-launch step: K blocks, several wide tiles of a round per block
# ---------------------------------------------------------------------------
@both
def test_one_launch_step_every_form(dev, libs, grid):
    """Every form of fa_fedavg_rounds_form (bf16: both outputs and the bf16 one
    alone), fa_fedavg_f16_rounds_form and fa_fedavg_f64_rounds_form over three
    rounds whose starts are multiples of the slot alignment, the last round
    ragged.  Before the first launch of a form: its step table at K blocks and
    these offsets covers every column once (small_grid.step_coverage)."""
    _lib, L, B = libs
    K, N, w = grid
    st = _stream(dev)
    n = SG.form_names(B)
    fams = [("f32", [x for x in n["step_forms"] if x.startswith("f32")], n["step_forms"]),
            ("bf16", [x for x in n["step_forms"] if x.startswith("bf16")], n["step_forms"]),
            ("f16", n["step_forms_f16"], n["step_forms_f16"]), ("f64", n["step_forms_f64"], n["step_forms_f64"])]
    assert sum(len(f[1]) for f in fams) == len(n["step_forms"]) + len(n["step_forms_f16"]) + len(n["step_forms_f64"])
    rb = ctypes.c_void_p()
    _lib.check(B.fa_bench_rounds_create(ctypes.byref(rb), dev.index or 0), "rounds state", bench=True)
    try:
        for kind, names, table in fams:
            _, _, P, T = _shape(libs, grid, kind)
            offsets = SG.step_offsets(kind, P)
            assert all(x % 64 == 0 for x in offsets[:-1]) and offsets[-1] == P and (w == 0 or P % SG.UNIT[kind])
            for x in names:
                count, held = SG.step_coverage(x, offsets, K)
                assert (count == 1).all() and held >= 2, (x, offsets, held)
            offs = (ctypes.c_int64 * 4)(*offsets)
            W = (P + 63) // 64 * 64
            buf, X = _stacked(dev, SG.matrix(kind, N, P), W)
            dt = {"f32": torch.float32, "bf16": torch.float32, "f16": torch.int16, "f64": torch.float64}[kind]
            for fid, a, s, d, exp in _cases(kind, N, P, T):
                ad, sd, sp = _factors(dev, a, s)
                o = _outs(dev, len(names), P, dt)
                ob, ob1 = (_outs(dev, len(names), P, torch.int16), _outs(dev, len(names), P, torch.int16)) \
                    if kind == "bf16" else (None, None)
                for k, x in enumerate(names):
                    f = table.index(x)
                    if kind == "f16":
                        rc = B.fa_fedavg_f16_rounds_form(rb, f, X.data_ptr(), N, W, ad.data_ptr(), sp, _half_bits(d),
                                                         o[k].data_ptr(), 3, offs, None, st)
                    elif kind == "f64":
                        rc = B.fa_fedavg_f64_rounds_form(rb, f, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d),
                                                         o[k].data_ptr(), 3, offs, None, st)
                    else:
                        rc = B.fa_fedavg_rounds_form(rb, f, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d),
                                                     o[k].data_ptr(), ob[k].data_ptr() if ob is not None else None, 3,
                                                     offs, st)
                    _lib.check(rc, x, bench=True)
                    if kind == "bf16":
                        _lib.check(B.fa_fedavg_rounds_form(rb, f, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d), None,
                                                           ob1[k].data_ptr(), 3, offs, st), x + " bf16 only", bench=True)
                torch.cuda.synchronize()
                what = (fid, K, N, P)
                if kind == "bf16":
                    _check(o, names, exp[0], P, what + ("fp32 out",))
                    _check(ob, names, exp[1], P, what + ("bf16 out",), nan16=0x7F80)
                    _check(ob1, names, exp[1], P, what + ("bf16 out alone",), nan16=0x7F80)
                else:
                    _check(o, names, exp, P, what, nan16=0x7C00 if kind == "f16" else None)
        assert L.fa_rounds_timeouts(rb) == 0
    finally:
        torch.cuda.synchronize()
        _lib.check(B.fa_bench_rounds_destroy(rb), "destroy", bench=True)
