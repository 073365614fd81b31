"""Every kernel the fp8 / MX family can launch runs once against the oracle:
source format x result x scored x per-client-scaled x source layout x path for
the single folds (fa_fedavg_fp8[_q][_ptrs], fa_fedavg_mx[_q][_ptrs]), source x
result x scored x scaled for the layer tables (fa_fedavg_mx_layers,
fa_fedavg_mx_q_layers; every launch takes both paths).

The specification is the parity files': the committed float32 oracle over the
rows dequantised on the CPU, and test_gpu_mx_out.py's _quantise of its
quotients.  Every input carries a block with a NaN and one with an infinity, so
the dead-block rule (E = 255, zero codes) is part of every quantising case.
Bit patterns and bytes are compared; no tolerance.
"""
import functools

import numpy as np
import pytest

import mx_cases as C
import test_gpu_fp8 as F8
import test_gpu_mx as M
import test_gpu_mx_out as MQ
from fedlesscan_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SOURCES = ["e4m3fn", "e5m2", "mx_e4m3", "mx_e5m2", "mx_e2m1"]
RESULTS = ["f32", "bf16", "both", "q_e4m3", "q_e5m2", "q_e2m1"]
# (layout, path): a stacked matrix / a row table on the vector path; the matrix starting one byte off / a
# table with one row a byte off on the one-column path
LAYOUTS = ["stacked", "table", "stacked_off", "table_odd_row"]
LAYERS = [64, 30, 70]  # aligned; the middle data row a byte off (one column per lane); aligned


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _shapes(src):
    """(N, P, a column of the NaN block, a column of the infinity block)."""
    if src.startswith("mx_"):
        return [(N, 70, 7, 66) for N in (3, M.AHEAD[src[3:]] + 2)]
    # 54: the last full unit's block (columns 32 .. 47) runs into the trailing columns, where its NaN sits;
    # 70: the trailing columns are a block of their own
    return [(N, P, *cols) for N in (3, F8.U + 2) for P, cols in ((54, (50, 51)), (70, (7, 66)))]


@functools.lru_cache(maxsize=None)
def _case(src, N, P, nan_col, inf_col, scored, scaled):
    """(element bytes, scale bytes or None, (float32, bf16 bits) of the oracle, factors)."""
    w, sc, scales = M._factors(N, scored, scaled)
    if src.startswith("mx_"):
        q, E, dead = C.with_dead_blocks(src, *M._bytes(src[3:], N, P), nan_col, inf_col)
        exp = M._oracle(src[3:], q, E, w, sc, scales)
    else:
        q, E, dead = C.with_dead_blocks(src, F8._bytes(src, N, P), None, nan_col, inf_col)
        exp = F8._oracle(src, q, w, sc, scales)
    bad = ~np.isfinite(exp[0])
    assert sorted({int(c) // 32 for c in np.flatnonzero(bad)}) == dead and 0 < len(dead) < (P + 31) // 32
    assert (exp[0][~bad] != 0).any()
    return q, E, exp, (w, sc, scales)


def _off_by_one(b, dev, dtype):
    """The byte rows as a matrix at a 16-byte pitch that starts one byte off a 16-byte boundary."""
    N, n = b.shape
    ld = (n + 15) // 16 * 16 + 16
    buf = torch.zeros(N * ld + 1, dtype=torch.uint8, device=dev)
    X = buf[1:].view(N, ld)[:, :n]
    X.copy_(torch.from_numpy(np.array(b)).to(dev))
    assert X.data_ptr() % 16 == 1
    return X.view(dtype)


def _rowset(src, q, E, layout, dev):
    """The rows as fold_stacked's arguments (matrix, block_scales or None) or as a RowSet whose placement
    is what the layout names."""
    from fedlesscan_amd import engine
    mx = src.startswith("mx_")
    dt = M.FMTS[src[3:]] if mx else F8.FMTS[src]
    if layout.startswith("stacked"):
        if layout == "stacked":
            X = M._place(q, "pitched", dev, dt, 16)
            assert X.data_ptr() % 16 == 0 and X.stride(0) % 16 == 0
        else:
            X = _off_by_one(q, dev, dt)
        return X, (M._place(E, "pitched", dev, torch.float8_e8m0fnu, 3) if mx else None)
    rows = M._place(q, layout, dev, dt, 16)
    rs = engine.RowSet(rows, M._place(E, "table_odd_row", dev, torch.float8_e8m0fnu, 3) if mx else None)
    assert rs.ptrs is not None and rs.view is None and rs.aligned == (layout == "table")
    return rs, None


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("result", RESULTS)
@pytest.mark.parametrize("src", SOURCES)
def test_single_fold(dev, src, result, scored, scaled, layout):
    from fedlesscan_amd import engine
    mx, out = src.startswith("mx_"), (result[2:] if result.startswith("q_") else None)
    for N, P, nan_col, inf_col in _shapes(src):
        q, E, exp, (w, sc, scales) = _case(src, N, P, nan_col, inf_col, scored, scaled)
        rows, es = _rowset(src, q, E, layout, dev)
        kw = dict(scales=scales) if es is None else dict(scales=scales, block_scales=es)
        fold = engine.fold_rows if isinstance(rows, engine.RowSet) else engine.fold_stacked
        what = f"N={N}, P={P}"
        before = dict(engine.stats)
        if out is not None:
            f32 = torch.zeros(P + 4, dtype=torch.float32, device=dev)
            got = fold(rows, w, sc, out_format=M.FMTS[out], out=f32[:P], **kw)
            MQ._same_mx(got, exp[0], out, what)
            M._same(f32[:P], exp, f"{what}: out=")
            assert not f32[P:].any()
        elif result == "f32":
            M._same(fold(rows, w, sc, **kw), exp, what)
        elif result == "bf16":
            ob = torch.zeros(P + 8, dtype=torch.bfloat16, device=dev)
            got = fold(rows, w, sc, out_bf16=ob[:P], **kw)
            assert got.dtype == torch.bfloat16 and got.data_ptr() == ob.data_ptr() and not ob[P:].any()
            M._same(got, exp, what)
        else:
            f, h = fold(rows, w, sc, want_bf16=True, **kw)
            M._same(f, exp, f"{what}: float32 of both")
            M._same(h, exp, f"{what}: bf16 of both")
        delta = {k: engine.stats[k] - before[k] for k in ("fp8_folds", "mx_folds", "mx_out_folds", "mx_table_folds")}
        assert delta == {"fp8_folds": int(not mx), "mx_folds": int(mx), "mx_out_folds": int(out is not None),
                         "mx_table_folds": 0}, what


# ---------------------------------------------------------------------------
# the layer tables
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_case(fmt, scored, scaled):
    """Per layer (element bytes, scale bytes, oracle, client scales or None); the 30-column layer is dead in
    the scored cases, so its one-column path meets the rule too."""
    N = 3
    w, sc, _ = M._factors(N, scored, False)
    res = []
    for k, P in enumerate(LAYERS):
        q, E = M._bytes(fmt, N + k, P)
        q, E = q[:N], E[:N]
        dead = []
        if k != 1 or scored:
            q, E, dead = C.with_dead_blocks("mx_" + fmt, q, E, 40 if k == 0 else 7, 40 if k == 0 else P - 4)
        cs = [c * (1 + k / 8) for c in M._factors(N, False, True)[2]] if scaled else None
        exp = M._oracle(fmt, q, E, w, sc, cs)
        assert sorted({int(c) // 32 for c in np.flatnonzero(~np.isfinite(exp[0]))}) == dead
        res.append((q, E, exp, cs))
    return res, w, sc


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("result", RESULTS)
@pytest.mark.parametrize("fmt", list(M.FMTS))
def test_layer_table(dev, fmt, result, scored, scaled):
    from fedlesscan_amd import MXLayer, engine
    layers, w, sc = _layer_case(fmt, scored, scaled)
    out = result[2:] if result.startswith("q_") else None
    cols = []
    for k, (q, E, _, cs) in enumerate(layers):
        rows = M._place(q, "table_odd_row" if k == 1 else "table", dev, M.FMTS[fmt], 16)
        es = M._place(E, "table_odd_row", dev, torch.float8_e8m0fnu, 3)
        cols.append([MXLayer(r, e, c) for r, e, c in zip(rows, es, cs or [None] * 3)])
    ms = engine.ModelRowSet([[col[i] for col in cols] for i in range(3)])
    assert ms.host_plan[:, 3].tolist() == [1, 0, 1] and ms.host_plan[:, 0].tolist() == LAYERS
    before = dict(engine.stats)
    if out is not None:
        f32 = torch.zeros(ms.elems, dtype=torch.float32, device=dev)
        got = engine.fold_model_rows(ms, w, sc, out_format=M.FMTS[out], out=f32)
        for k, (P, o) in enumerate(zip(LAYERS, ms.offsets)):
            MQ._same_mx(got[k], layers[k][2][0], out, f"layer {k}")
            M._same(f32[o:o + P], layers[k][2], f"out=, layer {k}")
            assert not f32[o + P:o + (P + 63) // 64 * 64].any()
    elif result == "f32":
        got = engine.fold_model_rows(ms, w, sc)
        for k in range(3):
            M._same(got[k], layers[k][2], f"layer {k}")
    elif result == "bf16":
        ob = torch.zeros(ms.elems, dtype=torch.bfloat16, device=dev)
        got = engine.fold_model_rows(ms, w, sc, out_bf16=ob)
        for k, (P, o) in enumerate(zip(LAYERS, ms.offsets)):
            assert got[k].dtype == torch.bfloat16 and got[k].data_ptr() == ob.data_ptr() + 2 * o
            M._same(got[k], layers[k][2], f"layer {k}")
            assert not ob[o + P:o + (P + 63) // 64 * 64].any()
    else:
        f, h = engine.fold_model_rows(ms, w, sc, want_bf16=True)
        for k in range(3):
            M._same(f[k], layers[k][2], f"float32 of both, layer {k}")
            M._same(h[k], layers[k][2], f"bf16 of both, layer {k}")
    delta = {k: engine.stats[k] - before[k] for k in ("fp8_folds", "mx_folds", "mx_out_folds", "mx_table_folds")}
    assert delta == {"fp8_folds": 0, "mx_folds": 3, "mx_out_folds": 3 * int(out is not None), "mx_table_folds": 1}


def test_the_matrix_is_the_launchers_whole_dispatch():
    """The parametrisation above, counted: what launch_mx[_q], launch_fp8[_q] and mx[_q]_layers_fold select
    from is source x result x scored x scaled x (pitched | table) x (vector | one column)."""
    single = {(s, r, sc, cs, lay.split("_")[0], "one column" if "_" in lay else "vector")
              for s in SOURCES for r in RESULTS for sc in (0, 1) for cs in (0, 1) for lay in LAYOUTS}
    assert len(single) == 5 * 6 * 2 * 2 * 2 * 2 == 480
    table = {(f, r, sc, cs, path) for f in M.FMTS for r in RESULTS for sc in (0, 1) for cs in (0, 1)
             for path in ("vector", "one column")}
    assert len(table) == 3 * 6 * 2 * 2 * 2 == 144
    assert _lib.FA_FP8_ROWS_AHEAD + 2 in {N for N, *_ in _shapes("e5m2")}
    assert _lib.FA_MX_ROWS_AHEAD_FP4 + 2 in {N for N, *_ in _shapes("mx_e2m1")}
