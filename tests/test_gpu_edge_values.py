"""Edge-value parity of every fold kernel form: signed zeros, subnormals,
overflow in client order, inf, NaN, zero weights and the bf16 rounding ties
(tests/edge_values.py), bit for bit against the C oracle, which
tests/test_edge_values_host.py proves against the literal numpy left fold on
these very inputs.  NaN is compared by position (the GPU's default NaN has the
other sign than x86's); every other element by its bits, -0.0 included.

The shapes are small: shapes, alignments and tails are covered elsewhere.  Here
each kernel runs its distinct arithmetic paths (first-row initialisation, the
row-group loop and its remainder, partial and pipelined LDS chunks, clamped
lanes, the column tail, continue-from-accumulator, finalise) on values that a
zero-initialised accumulator, a flushed subnormal, a skipped or manufactured
zero-weight term, a fused multiply-add, another summation order or a wrong
bf16 rounding would change.  Outputs are NaN-filled before each launch, so an
element that is never written fails too."""
import ctypes
import functools

import numpy as np
import pytest

import edge_values as E
import golden_cases as G
from oracle import oracle_lib as OL  # checker

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 2024
# every client count once, every width twice: one row; two rows; a row group and its
# remainder (8 + 1, 32 + 1); two full LDS chunks and a partial one; the 8-wave forms (N >= 256)
SHAPES = [(1, 7), (2, 1027), (9, 1027), (33, 4099), (70, 4099), (300, 1027)]
SENT16 = 0x5A5A  # a bf16 output element no kernel writes keeps this pattern


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def libs():
    from fedlesscan_amd import _lib
    return _lib, _lib.load(), _lib.load_bench()


# ---------------------------------------------------------------------------
# inputs and expectations, made once per shape and shared, never modified
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix(kind, N, P):
    X = {"f32": E.matrix_f32, "bf16": E.matrix_bf16, "f64": E.matrix_f64}[kind](SEED, N, P)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _cases(kind, N, P):
    """[(id, a, s or None, divisor, expected)]: every factor set, plain and
    scored; expected = the oracle's output (bf16: (fp32, bf16 bits))."""
    X = _matrix(kind, N, P)
    out = []
    for name, a, s, d in E.factor_sets(SEED, N, np.float64 if kind == "f64" else np.float32):
        if kind == "f32":
            exp = OL.fedavg_f32(X, a, d, s=s)
        elif kind == "f64":
            exp = OL.fedavg_f64(X, a, d, s=s)
        else:
            exp = OL.fedavg_bf16(X, a, d, s=s)
        out.append((E.set_id(name, s), a, s, d, exp))
    assert len(out) == 2 * len(E.FACTOR_SETS)
    return out


def _dev_factors(dev, a, s):
    ad = torch.from_numpy(a.copy()).to(dev)
    sd = None if s is None else torch.from_numpy(s.copy()).to(dev)
    return ad, sd, (None if sd is None else sd.data_ptr())


def _stacked(dev, Xh, ldx, off=0):
    """The rows of Xh at pitch ldx, the first at element `off` of a buffer whose
    every other element is NaN (pitch padding is never to be read into a
    result).  Returns (buffer, [N, P] view)."""
    N, P = Xh.shape
    if Xh.dtype == np.uint16:
        buf = torch.full((N * ldx + off + 8,), 0x7FC0, dtype=torch.int16, device=dev)
        src = torch.from_numpy(Xh.view(np.int16).copy())
    else:
        buf = torch.full((N * ldx + off + 8,), float("nan"), dtype=torch.from_numpy(Xh[:0].copy()).dtype, device=dev)
        src = torch.from_numpy(Xh.copy())
    view = buf[off:off + N * ldx].view(N, ldx)[:, :P]
    view.copy_(src.to(dev))
    return buf, view


def _outs(dev, n, P, dtype=torch.float32, align=16):
    """n output rows of P elements, each 16-B aligned, NaN-filled, with NaN padding behind each."""
    per = align // torch.empty(0, dtype=dtype).element_size()
    w = (P + per - 1) // per * per + per
    return torch.full((n, w), float("nan"), dtype=dtype, device=dev)


def _outs16(dev, n, P):
    w = (P + 7) // 8 * 8 + 8
    return torch.full((n, w), SENT16, dtype=torch.int16, device=dev)


def _check32(h, names, exp, P, what):
    """h: [len(names), w] host array of outputs launched into _outs rows."""
    assert h.shape[0] == len(names)
    for k, name in enumerate(names):
        assert G.same_bits(h[k, :P], exp), (name,) + what
        assert np.isnan(h[k, P:]).all(), ("wrote behind out", name) + what


def _check16(hb, names, exp, P, what):
    ef, eb = exp
    hb = hb.view(np.uint16)
    for k, name in enumerate(names):
        assert E.same_bf16_bits(hb[k, :P], eb), (name,) + what
        # and against a rounding that does not share the kernel's expression
        assert E.bf16_matches_independent(hb[k, :P], ef), ("independent rounding", name) + what
        assert (hb[k, P:] == SENT16).all(), ("wrote behind out_bf16", name) + what


def _separate_rows(dev, Xh, shift=0):
    """Each row its own allocation; shift = 1: every row one element past a 16-B boundary."""
    rows, keep = [], []
    tdt = torch.int16 if Xh.dtype == np.uint16 else None
    for i in range(Xh.shape[0]):
        src = torch.from_numpy((Xh[i].view(np.int16) if tdt else Xh[i]).copy())
        holder = torch.zeros(src.numel() + shift, dtype=src.dtype, device=dev)
        holder[shift:].copy_(src)
        keep.append(holder)
        rows.append(holder[shift:])
    assert all((r.data_ptr() % 16 == 0) == (shift == 0) for r in rows)
    tab = torch.tensor([r.data_ptr() for r in rows], dtype=torch.int64, device=dev)
    return rows, tab, keep


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------------------
# fp32 stacked: every variant, every product form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", SHAPES)
def test_f32_every_variant_and_form(dev, libs, N, P):
    """fa_fedavg_f32_variant (variant 0 = the product's fa_fedavg_f32) and
    fa_fedavg_f32_form on 16-B aligned rows with a padded pitch."""
    _lib, L, B = libs
    ldx = (P + 3) // 4 * 4 + 4
    buf, X = _stacked(dev, _matrix("f32", N, P), ldx)
    st = _stream(dev)
    vnames = [B.fa_variant_name(v).decode() for v in range(B.fa_num_variants())]
    fnames = ["form " + B.fa_f32_form_name(f).decode() for f in range(B.fa_num_f32_forms())]
    assert len(set(vnames)) == len(vnames) and all(vnames) and all(n != "form " for n in fnames)
    ran = set()
    for fid, a, s, d, exp in _cases("f32", N, P):
        ad, sd, sp = _dev_factors(dev, a, s)
        o = _outs(dev, len(vnames) + len(fnames), P)
        for v in range(len(vnames)):
            _lib.check(B.fa_fedavg_f32_variant(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, float(d), o[v].data_ptr(),
                                               st, v), vnames[v], bench=True)
            ran.add(vnames[v])
        for f in range(len(fnames)):
            _lib.check(B.fa_fedavg_f32_form(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, float(d),
                                            o[len(vnames) + f].data_ptr(), st, f), fnames[f], bench=True)
            ran.add(fnames[f])
        _check32(o.cpu().numpy(), vnames + fnames, exp, P, (fid, N, P))
    assert len(ran) >= B.fa_num_variants() + B.fa_num_f32_forms()


@pytest.mark.parametrize("N,P", [(2, 7), (9, 1027), (70, 4099), (300, 1027)])
def test_f32_any_alignment_variants(dev, libs, N, P):
    """The 4-byte-load LDS folds, the scalar fold and the product entry on an
    odd row pitch, the first row one float past a 16-B boundary, into an output
    at a 4-byte offset."""
    _lib, L, B = libs
    pitch = P + 2 if P % 2 else P + 1
    buf, X = _stacked(dev, _matrix("f32", N, P), pitch, off=1)
    assert X.data_ptr() % 16 == 4 and pitch % 2 == 1
    st = _stream(dev)
    vs = [v for v in range(B.fa_num_variants()) if B.fa_variant_name(v).startswith((b"dw_", b"scalar", b"pm_dw_"))]
    assert len(vs) >= 9
    names = ["fa_fedavg_f32"] + [B.fa_variant_name(v).decode() for v in vs]
    for fid, a, s, d, exp in _cases("f32", N, P):
        ad, sd, sp = _dev_factors(dev, a, s)
        o = _outs(dev, len(names), P + 1)
        _lib.check(L.fa_fedavg_f32(X.data_ptr(), N, P, pitch, ad.data_ptr(), sp, float(d), o[0, 1:].data_ptr(), st),
                   "fa_fedavg_f32")
        for k, v in enumerate(vs):
            _lib.check(B.fa_fedavg_f32_variant(X.data_ptr(), N, P, pitch, ad.data_ptr(), sp, float(d),
                                               o[k + 1, 1:].data_ptr(), st, v), names[k + 1], bench=True)
        h = o.cpu().numpy()
        assert np.isnan(h[:, 0]).all(), "wrote before out"
        _check32(h[:, 1:], names, exp, P, (fid, N, P))


# ---------------------------------------------------------------------------
# fp32 pointer-table folds
# ---------------------------------------------------------------------------
PTR_SHAPES = [(1, 7), (9, 1027), (70, 4099), (300, 1027)]


@pytest.mark.parametrize("N,P", PTR_SHAPES)
def test_f32_row_table_aligned_rows(dev, libs, N, P):
    """Separately allocated 16-B aligned rows: every fa_fedavg_f32_ptrs_variant,
    every fa_fedavg_f32_ptrs_form, the product's two entries and
    engine.fold_rows through a RowSet."""
    from fedlesscan_amd import engine
    _lib, L, B = libs
    rows, tab, _keep = _separate_rows(dev, _matrix("f32", N, P))
    rs = engine.RowSet(rows)
    assert rs.view is None and rs.aligned
    st = _stream(dev)
    vnames = [B.fa_ptrs_variant_name(v).decode() for v in range(B.fa_num_ptrs_variants())]
    fnames = ["form " + B.fa_ptrs_form_name(f).decode() for f in range(B.fa_num_ptrs_forms())]
    names = vnames + fnames + ["fa_fedavg_f32_ptrs_aligned", "fa_fedavg_f32_ptrs", "fold_rows"]
    assert len(set(names)) == len(names) and all(vnames)
    ran = 0
    for fid, a, s, d, exp in _cases("f32", N, P):
        ad, sd, sp = _dev_factors(dev, a, s)
        o = _outs(dev, len(names), P)
        k = 0
        for v in range(len(vnames)):
            _lib.check(B.fa_fedavg_f32_ptrs_variant(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d),
                                                    o[k].data_ptr(), st, v), vnames[v], bench=True)
            k += 1
        for f in range(len(fnames)):
            _lib.check(B.fa_fedavg_f32_ptrs_form(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), o[k].data_ptr(),
                                                 st, f), fnames[f], bench=True)
            k += 1
        _lib.check(L.fa_fedavg_f32_ptrs_aligned(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), o[k].data_ptr(),
                                                st), names[k])
        _lib.check(L.fa_fedavg_f32_ptrs(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), o[k + 1].data_ptr(), st),
                   names[k + 1])
        engine.fold_rows(rs, a.tolist(), None if s is None else s.tolist(), total=float(d), out=o[k + 2, :P])
        ran = max(ran, k)
        _check32(o.cpu().numpy(), names, exp, P, (fid, N, P))
    assert ran >= B.fa_num_ptrs_variants() + B.fa_num_ptrs_forms()


@pytest.mark.parametrize("N,P", PTR_SHAPES)
def test_f32_row_table_rows_at_a_4_byte_offset(dev, libs, N, P):
    """Rows one float past a 16-B boundary: the any-alignment pointer variants,
    fa_fedavg_f32_ptrs and engine.fold_rows through a RowSet, the output at a
    4-byte offset too."""
    from fedlesscan_amd import engine
    _lib, L, B = libs
    rows, tab, _keep = _separate_rows(dev, _matrix("f32", N, P), shift=1)
    rs = engine.RowSet(rows)
    assert rs.view is None and not rs.aligned
    st = _stream(dev)
    vs = [v for v in range(B.fa_num_ptrs_variants())
          if B.fa_ptrs_variant_name(v).startswith((b"ptrs_dw", b"ptrs_rows_scalar", b"ptrs_generic"))]
    assert len(vs) >= 6
    names = ["fa_fedavg_f32_ptrs", "fold_rows"] + [B.fa_ptrs_variant_name(v).decode() for v in vs]
    for fid, a, s, d, exp in _cases("f32", N, P):
        ad, sd, sp = _dev_factors(dev, a, s)
        o = _outs(dev, len(names), P + 1)
        _lib.check(L.fa_fedavg_f32_ptrs(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d), o[0, 1:].data_ptr(), st),
                   names[0])
        engine.fold_rows(rs, a.tolist(), None if s is None else s.tolist(), total=float(d), out=o[1, 1:P + 1])
        for k, v in enumerate(vs):
            _lib.check(B.fa_fedavg_f32_ptrs_variant(tab.data_ptr(), N, P, ad.data_ptr(), sp, float(d),
                                                    o[k + 2, 1:].data_ptr(), st, v), names[k + 2], bench=True)
        h = o.cpu().numpy()
        assert np.isnan(h[:, 0]).all(), "wrote before out"
        _check32(h[:, 1:], names, exp, P, (fid, N, P))


# ---------------------------------------------------------------------------
# chunked and streaming folds: the accumulator round-trips through memory
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", [(2, 7), (9, 1027), (33, 4099), (300, 1027)])
@pytest.mark.parametrize("layout", ["vector", "odd_pitch"])
def test_f32_chunked_fold_in_place(dev, libs, N, P, layout):
    """fa_fold_f32 in three cuts, the accumulator carried in place (acc_in ==
    out): a -0.0, a subnormal, an inf or a NaN partial sum must survive the
    round trip through memory, and only the last cut divides."""
    _lib, L, B = libs
    if layout == "vector":
        ldx, off = (P + 3) // 4 * 4 + 4, 0
    else:
        ldx, off = (P + 2 if P % 2 else P + 1), 1
    buf, X = _stacked(dev, _matrix("f32", N, P), ldx, off)
    st = _stream(dev)
    cuts = sorted({0, min(1, N), (N + 1) // 2, N})
    cases = _cases("f32", N, P)
    o = _outs(dev, len(cases), P + 1)
    shift = 0 if layout == "vector" else 1
    for k, (fid, a, s, d, exp) in enumerate(cases):
        ad, sd, sp = _dev_factors(dev, a, s)
        acc = o[k, shift:]
        for c, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
            _lib.check(L.fa_fold_f32(X[r0].data_ptr(), r1 - r0, P, ldx, ad[r0:].data_ptr(),
                                     None if sd is None else sd[r0:].data_ptr(), None if c == 0 else acc.data_ptr(),
                                     float(d), int(r1 == N), acc.data_ptr(), st), "fa_fold_f32")
    h = o.cpu().numpy()
    for k, (fid, a, s, d, exp) in enumerate(cases):
        _check32(h[k:k + 1, shift:], ["fa_fold_f32 " + layout], exp, P, (fid, N, P, cuts))
    assert shift == 0 or np.isnan(h[:, 0]).all()


@pytest.mark.parametrize("N,P", [(1, 7), (9, 1027), (33, 4099)])
def test_f32_accumulate_and_finalize_row_by_row(dev, libs, N, P):
    """fa_accumulate_f32 per client (s = 1 for the plain fold: exact), then
    fa_finalize_f32 into another buffer and in place."""
    _lib, L, B = libs
    buf, X = _stacked(dev, _matrix("f32", N, P), P)
    st = _stream(dev)
    cases = _cases("f32", N, P)
    o = _outs(dev, 2 * len(cases), P)
    for k, (fid, a, s, d, exp) in enumerate(cases):
        acc = o[2 * k]
        for i in range(N):
            _lib.check(L.fa_accumulate_f32(acc.data_ptr(), X[i].data_ptr(), float(a[i]),
                                           1.0 if s is None else float(s[i]), int(i == 0), P, st), "fa_accumulate_f32")
        _lib.check(L.fa_finalize_f32(acc.data_ptr(), float(d), o[2 * k + 1].data_ptr(), P, st), "fa_finalize_f32")
        _lib.check(L.fa_finalize_f32(acc.data_ptr(), float(d), acc.data_ptr(), P, st), "fa_finalize_f32 in place")
    h = o.cpu().numpy()
    for k, (fid, a, s, d, exp) in enumerate(cases):
        _check32(h[2 * k:2 * k + 2], ["finalize in place", "finalize"], exp, P, (fid, N, P))


# ---------------------------------------------------------------------------
# host-factor entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", [(9, 1027), (70, 4099)])
def test_host_factor_entries(dev, libs, N, P):
    """fa_fedavg_f32_hostf (vector layout and odd pitch), fa_fedavg_f32_ptrs_hostf,
    fa_fedavg_bf16_hostf and fa_fedavg_bf16_ptrs_hostf (rows promised aligned
    and not): the factors, zeros and fractions included, staged by the library."""
    _lib, L, B = libs
    st = _stream(dev)
    ldx = (P + 3) // 4 * 4 + 4
    _b1, Xv = _stacked(dev, _matrix("f32", N, P), ldx)
    pitch = P + 2 if P % 2 else P + 1
    _b2, Xo = _stacked(dev, _matrix("f32", N, P), pitch, off=1)
    rows, tab, _k1 = _separate_rows(dev, _matrix("f32", N, P))
    ldb = (P + 7) // 8 * 8 + 8
    _b3, Xb = _stacked(dev, _matrix("bf16", N, P), ldb)
    rows16, tab16, _k2 = _separate_rows(dev, _matrix("bf16", N, P))
    n32 = ["f32_hostf", "f32_hostf odd pitch", "f32_ptrs_hostf aligned", "f32_ptrs_hostf"]
    n16 = ["bf16_hostf", "bf16_hostf bf16 only", "bf16_ptrs_hostf aligned", "bf16_ptrs_hostf",
           "bf16_ptrs_hostf bf16 only"]
    for (fid, a, s, d, exp), (_, _, _, _, exp16) in zip(_cases("f32", N, P), _cases("bf16", N, P)):
        a, s = a.copy(), None if s is None else s.copy()
        ap, sp, dv = a.ctypes.data, None if s is None else s.ctypes.data, float(d)
        o = _outs(dev, len(n32), P)
        _lib.check(L.fa_fedavg_f32_hostf(Xv.data_ptr(), N, P, ldx, ap, sp, dv, o[0].data_ptr(), st), n32[0])
        _lib.check(L.fa_fedavg_f32_hostf(Xo.data_ptr(), N, P, pitch, ap, sp, dv, o[1].data_ptr(), st), n32[1])
        _lib.check(L.fa_fedavg_f32_ptrs_hostf(tab.data_ptr(), N, P, ap, sp, dv, 1, o[2].data_ptr(), st), n32[2])
        _lib.check(L.fa_fedavg_f32_ptrs_hostf(tab.data_ptr(), N, P, ap, sp, dv, 0, o[3].data_ptr(), st), n32[3])
        of = _outs(dev, len(n16), P)
        ob = _outs16(dev, len(n16), P)
        _lib.check(L.fa_fedavg_bf16_hostf(Xb.data_ptr(), N, P, ldb, ap, sp, dv, of[0].data_ptr(), ob[0].data_ptr(), st),
                   n16[0])
        _lib.check(L.fa_fedavg_bf16_hostf(Xb.data_ptr(), N, P, ldb, ap, sp, dv, None, ob[1].data_ptr(), st), n16[1])
        _lib.check(L.fa_fedavg_bf16_ptrs_hostf(tab16.data_ptr(), N, P, ap, sp, dv, 1, of[2].data_ptr(),
                                               ob[2].data_ptr(), st), n16[2])
        _lib.check(L.fa_fedavg_bf16_ptrs_hostf(tab16.data_ptr(), N, P, ap, sp, dv, 0, of[3].data_ptr(),
                                               ob[3].data_ptr(), st), n16[3])
        _lib.check(L.fa_fedavg_bf16_ptrs_hostf(tab16.data_ptr(), N, P, ap, sp, dv, 1, None, ob[4].data_ptr(), st),
                   n16[4])
        a[:] = -7.0  # the library copied them
        if s is not None:
            s[:] = 3.0
        _check32(o.cpu().numpy(), n32, exp, P, (fid, N, P))
        hf = of.cpu().numpy()
        for k in (0, 2, 3):
            _check32(hf[k:k + 1], [n16[k]], exp16[0], P, (fid, N, P))
        assert np.isnan(hf[[1, 4]]).all(), "an fp32 store without an fp32 output"
        _check16(ob.cpu().numpy(), n16, exp16, P, (fid, N, P))


# ---------------------------------------------------------------------------
# bf16: stacked variants and forms, row-table forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", SHAPES)
def test_bf16_every_variant_and_form(dev, libs, N, P):
    """fa_fedavg_bf16_variant (variant 0 = the product's fa_fedavg_bf16) and
    fa_fedavg_bf16_form, with both outputs and with the bf16 output alone: the
    fp32 bits, and the bf16 bits at the ties, at the overflow to inf, on
    subnormal results, on -0 and on NaN."""
    _lib, L, B = libs
    ldx = (P + 7) // 8 * 8 + 8
    buf, X = _stacked(dev, _matrix("bf16", N, P), ldx)
    st = _stream(dev)
    vnames = [B.fa_bf16_variant_name(v).decode() for v in range(B.fa_num_bf16_variants())]
    fnames = ["form " + B.fa_bf16_form_name(f).decode() for f in range(B.fa_num_bf16_forms())]
    names = vnames + fnames
    assert len(set(names)) == len(names) and all(vnames)
    n = len(names)

    def launch(k, ad, sp, d, of, ob):
        if k < len(vnames):
            rc = B.fa_fedavg_bf16_variant(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, d, of, ob, st, k)
        else:
            rc = B.fa_fedavg_bf16_form(X.data_ptr(), N, P, ldx, ad.data_ptr(), sp, d, of, ob, st, k - len(vnames))
        _lib.check(rc, names[k], bench=True)

    ran = set()
    for fid, a, s, d, exp in _cases("bf16", N, P):
        ad, sd, sp = _dev_factors(dev, a, s)
        of, ob, ob1 = _outs(dev, n, P), _outs16(dev, n, P), _outs16(dev, n, P)
        for k in range(n):
            launch(k, ad, sp, float(d), of[k].data_ptr(), ob[k].data_ptr())
            launch(k, ad, sp, float(d), None, ob1[k].data_ptr())
            ran.add(names[k])
        _check32(of.cpu().numpy(), names, exp[0], P, (fid, N, P))
        _check16(ob.cpu().numpy(), names, exp, P, (fid, N, P))
        _check16(ob1.cpu().numpy(), [x + " bf16 only" for x in names], exp, P, (fid, N, P))
    assert len(ran) >= B.fa_num_bf16_variants() + B.fa_num_bf16_forms()


@pytest.mark.parametrize("N,P", SHAPES)
def test_bf16_every_row_table_form(dev, libs, N, P):
    """fa_fedavg_bf16_ptrs_form: the octet forms (rows promised aligned), the
    column form (promised and not, and on rows at a 2-byte offset), the policy
    (-1, = fa_fedavg_bf16_ptrs), each with both outputs and with the bf16
    output alone; engine.fold_rows through a RowSet."""
    from fedlesscan_amd import engine
    _lib, L, B = libs
    Xh = _matrix("bf16", N, P)
    rows, tab, _k1 = _separate_rows(dev, Xh)
    rows_o, tab_o, _k2 = _separate_rows(dev, Xh, shift=1)
    rs = engine.RowSet([r.view(torch.bfloat16) for r in rows])
    assert rs.view is None and rs.aligned
    st = _stream(dev)
    runs = []  # (name, form, table, rows_aligned)
    nforms = B.fa_num_rows16_forms()
    for f in range(nforms):
        name = B.fa_rows16_form_name(f).decode()
        assert name
        runs.append((name, f, tab, 1))
        if name.endswith("column"):
            runs.append((name + " unpromised", f, tab, 0))
            runs.append((name + " 2-byte offset rows", f, tab_o, 0))
    runs += [("policy aligned", -1, tab, 1), ("policy", -1, tab, 0), ("policy 2-byte offset rows", -1, tab_o, 0)]
    assert len({f for _, f, _, _ in runs if f >= 0}) >= nforms and any(n.endswith("column") for n, *_ in runs)
    names = [r[0] for r in runs]
    n = len(runs)
    for fid, a, s, d, exp in _cases("bf16", N, P):
        ad, sd, sp = _dev_factors(dev, a, s)
        of, ob, ob1 = _outs(dev, n + 1, P), _outs16(dev, n + 1, P), _outs16(dev, n, P)
        for k, (name, f, t, al) in enumerate(runs):
            _lib.check(B.fa_fedavg_bf16_ptrs_form(t.data_ptr(), N, P, ad.data_ptr(), sp, float(d), al,
                                                  of[k].data_ptr(), ob[k].data_ptr(), st, f), name, bench=True)
            _lib.check(B.fa_fedavg_bf16_ptrs_form(t.data_ptr(), N, P, ad.data_ptr(), sp, float(d), al, None,
                                                  ob1[k].data_ptr(), st, f), name + " bf16 only", bench=True)
        engine.fold_rows(rs, a.tolist(), None if s is None else s.tolist(), total=float(d), out=of[n, :P],
                         out_bf16=ob[n, :P].view(torch.bfloat16))
        _check32(of.cpu().numpy(), names + ["fold_rows"], exp[0], P, (fid, N, P))
        _check16(ob.cpu().numpy(), names + ["fold_rows"], exp, P, (fid, N, P))
        _check16(ob1.cpu().numpy(), [x + " bf16 only" for x in names], exp, P, (fid, N, P))


# ---------------------------------------------------------------------------
# the one-launch step (write-through tile stores), agent scope, one process
# ---------------------------------------------------------------------------
# Three rounds that each hold a full tile of a step form and a last tile with
# exactly one octet: 8192 + 8 columns (4 octets per lane), 4096 + 8 (2 octets
# per lane), and 8192 + 8 + 3 (the same with a 3-column tail).
P_STEP_TILES = 8200 + 4104 + 8203


def _round_offsets(P):
    """Three small rounds, every start a multiple of 8, the last one ragged."""
    if P == P_STEP_TILES:
        return [0, 8200, 8200 + 4104, P]
    q = P // 4 // 8 * 8
    return [0, q, 3 * q, P] if q else [0, P]


# N = 1, 2 and 10 at P_STEP_TILES: the first row alone, no full row group, and
# one group of the step forms' 8 rows ahead with a leftover row
@pytest.mark.parametrize("N,P", [(9, 1027), (33, 4099), (70, 4099), (1, P_STEP_TILES), (2, P_STEP_TILES),
                                 (10, P_STEP_TILES)])
@pytest.mark.parametrize("bf16", [False, True])
def test_one_launch_step_every_form(dev, libs, N, P, bf16):
    """Every step form (fa_fedavg_rounds_form) and the product's
    fa_fedavg_f32_rounds / fa_fedavg_bf16_rounds over three rounds whose last
    ends off an octet boundary; bf16 with both outputs and the bf16 one alone.
    The columns behind the last round stay untouched."""
    _lib, L, B = libs
    kind = "bf16" if bf16 else "f32"
    W = (P + 63) // 64 * 64  # the row pitch, as sharding.ALIGN
    buf, X = _stacked(dev, _matrix(kind, N, P), W)
    offsets = _round_offsets(P)
    rounds = len(offsets) - 1
    assert rounds == 3 and all(o % 8 == 0 for o in offsets[:-1]) and P % 8
    offs = (ctypes.c_int64 * (rounds + 1))(*offsets)
    st = _stream(dev)
    forms = [f for f in range(B.fa_num_step_forms()) if B.fa_step_form_name(f).decode().startswith("bf16") == bf16]
    fnames = [B.fa_step_form_name(f).decode() for f in forms]
    assert len(forms) >= 2 and L.fa_rounds_form(int(bf16)).decode() in fnames
    # the two parametrisations together see every form the library reports
    other = [f for f in range(B.fa_num_step_forms()) if f not in forms]
    assert all(B.fa_step_form_name(f).decode().startswith("bf16") != bf16 for f in other)
    assert len(forms) + len(other) >= B.fa_num_step_forms() and all(fnames)
    names = fnames + ["product rounds"]
    n = len(names)
    rb, r = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(B.fa_bench_rounds_create(ctypes.byref(rb), dev.index or 0), "rounds state", bench=True)
    _lib.check(L.fa_rounds_create(ctypes.byref(r), dev.index or 0), "fa_rounds_create")
    try:
        for fid, a, s, d, exp in _cases(kind, N, P):
            ad, sd, sp = _dev_factors(dev, a, s)
            of = _outs(dev, n, P)
            ob, ob1 = (_outs16(dev, n, P), _outs16(dev, n, P)) if bf16 else (None, None)
            for k, f in enumerate(forms):
                _lib.check(B.fa_fedavg_rounds_form(rb, f, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d),
                                                   of[k].data_ptr(), ob[k].data_ptr() if bf16 else None, rounds, offs,
                                                   st), fnames[k], bench=True)
                if bf16:
                    _lib.check(B.fa_fedavg_rounds_form(rb, f, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d), None,
                                                       ob1[k].data_ptr(), rounds, offs, st), fnames[k] + " bf16 only",
                               bench=True)
            k = n - 1
            if bf16:
                _lib.check(L.fa_fedavg_bf16_rounds(r, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d),
                                                   of[k].data_ptr(), ob[k].data_ptr(), rounds, offs, None, st),
                           names[k])
                _lib.check(L.fa_fedavg_bf16_rounds(r, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d), None,
                                                   ob1[k].data_ptr(), rounds, offs, None, st), names[k] + " bf16 only")
            else:
                _lib.check(L.fa_fedavg_f32_rounds(r, X.data_ptr(), N, W, ad.data_ptr(), sp, float(d), of[k].data_ptr(),
                                                  rounds, offs, None, st), names[k])
            torch.cuda.synchronize()
            _check32(of.cpu().numpy(), names, exp[0] if bf16 else exp, P, (fid, N, P))
            if bf16:
                _check16(ob.cpu().numpy(), names, exp, P, (fid, N, P))
                _check16(ob1.cpu().numpy(), [x + " bf16 only" for x in names], exp, P, (fid, N, P))
        assert L.fa_rounds_timeouts(r) == 0 and L.fa_rounds_check(r) == 0
    finally:
        torch.cuda.synchronize()
        _lib.check(B.fa_bench_rounds_destroy(rb), "destroy", bench=True)
        _lib.check(L.fa_rounds_destroy(r), "fa_rounds_destroy")


# ---------------------------------------------------------------------------
# float64 and the integer entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", SHAPES)
def test_f64_both_kernels(dev, libs, N, P):
    """fa_fedavg_f64: the two-column kernel (16-B aligned rows, even pitch) and
    the scalar kernel, reached through a view at an 8-byte offset, on the
    classes at double's ranges."""
    _lib, L, B = libs
    Xh = _matrix("f64", N, P)
    ldx = (P + 1) // 2 * 2 + 2
    _b1, Xv = _stacked(dev, Xh, ldx)
    _b2, Xo = _stacked(dev, Xh, ldx + 1, off=1)
    assert Xv.data_ptr() % 16 == 0 and Xo.data_ptr() % 16 == 8
    st = _stream(dev)
    names = ["two-column", "scalar"]
    for fid, a, s, d, exp in _cases("f64", N, P):
        ad, sd, sp = _dev_factors(dev, a, s)
        o = _outs(dev, 2, P, torch.float64)
        _lib.check(L.fa_fedavg_f64(Xv.data_ptr(), N, P, ldx, ad.data_ptr(), sp, float(d), o[0].data_ptr(), st),
                   names[0])
        _lib.check(L.fa_fedavg_f64(Xo.data_ptr(), N, P, ldx + 1, ad.data_ptr(), sp, float(d), o[1].data_ptr(), st),
                   names[1])
        _check32(o.cpu().numpy(), names, exp, P, (fid, N, P))


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_integer_entries_wrap_as_numpy(dev, dt):
    """fa_fedavg_i32 / fa_fedavg_i64 through FedAvgAggregator._aggregate with
    values near the type's limits: `layer * n` and the running sum wrap in the
    integer dtype exactly as numpy's do (the kernels compute in unsigned), then
    true-divide into float64."""
    from fedlesscan_amd import FedAvgAggregator
    info = np.iinfo(dt)
    N, P = 9, 1027
    rng = np.random.default_rng([SEED, info.bits])
    near = np.array([info.max, info.min, info.max - 1, info.min + 1, info.max // 2 + 1, info.min // 2 - 1, -1, 0, 1],
                    dtype=dt)
    X = near[rng.integers(0, near.size, size=(N, P))]
    X[:, ::7] = rng.integers(info.min, info.max, size=(N, len(range(0, P, 7))), dtype=dt, endpoint=True)
    w = [3, 1, 7, 2, 600, 5, 1, 2, 9]
    params = [[X[i, :1000].reshape(10, 100).copy(), X[i, 1000:].copy()] for i in range(N)]
    exp = []
    for li in range(2):
        acc = None
        for i in range(N):
            t = np.multiply(params[i][li], w[i])
            acc = t if acc is None else np.add(acc, t)
        assert acc.dtype == dt
        exp.append(acc / sum(w))
    wrapped = np.concatenate([(X[i].astype(object) * w[i]) for i in range(N)])
    assert (wrapped > info.max).any() and (wrapped < info.min).any(), "the products must leave the type's range"
    got = FedAvgAggregator()._aggregate(params, w)
    assert len(got) == 2
    for g, e in zip(got, exp):
        assert g.dtype == np.float64 and g.shape == e.shape and G.same_bits(np.asarray(g), e)
