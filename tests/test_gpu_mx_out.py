"""GPU parity of the MX result of the MX and fp8 folds (fa_fedavg_mx_q,
fa_fedavg_fp8_q and their _ptrs entries) through engine.fold_stacked,
engine.fold_rows and engine.aggregate_layers.

The quotients are the committed float32 oracle's over the rows dequantised on
the CPU (test_gpu_mx.py / test_gpu_fp8.py form them); _quantise is DESIGN.md 2's
contract in numpy.  Codes and scale bytes are compared as bytes; no tolerance.
"""

import numpy as np
import pytest

import test_gpu_fp8 as F8
import test_gpu_mx as M
from fedlesscan_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = _lib.FA_MX_TILE_COLS
FMTS = M.FMTS
QF = {"e4m3": (8, 448.0), "e5m2": (15, 57344.0), "e2m1": (2, 6.0)}  # emax, maxnorm
MAGS = np.array([0, .5, 1, 1.5, 2, 3, 4, 6])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _quantise(v: np.ndarray, fmt: str):
    """(element bytes, scale bytes) of the float32 quotients v."""
    emax, maxnorm = QF[fmt]
    nb = (v.size + 31) // 32
    B = np.zeros(nb * 32, dtype=np.float32)
    B[:v.size] = v
    B = B.reshape(nb, 32)
    dead = ~np.isfinite(B).all(axis=1)
    amax = np.abs(np.where(np.isfinite(B), B, np.float32(0))).max(axis=1)
    E = np.where(dead, 255, np.maximum((amax.view(np.uint32) >> 23).astype(np.int64) - emax, 0))
    y = np.clip(B.astype(np.float64) / np.exp2((E - 127).astype(np.float64))[:, None], -maxnorm, maxnorm)
    y[dead] = 0.0
    if fmt == "e2m1":
        d = np.abs(np.abs(y)[..., None] - MAGS)
        c = d.argmin(-1)  # the lower code of a tie
        tie = (c < 7) & (np.take_along_axis(d, np.minimum(c + 1, 7)[..., None], -1)[..., 0] == d.min(-1))
        c = np.where(tie & (c % 2 == 1), c + 1, c) | (np.signbit(B) & ~dead[:, None]) << 3
        codes = (c[:, 0::2] | c[:, 1::2] << 4).astype(np.uint8).reshape(-1)[:v.size // 2]
    else:
        codes = torch.tensor(y, dtype=torch.float32).to(FMTS[fmt]).view(torch.uint8).numpy().reshape(-1)[:v.size]
    return codes, E.astype(np.uint8)


def _same_mx(got, v, fmt, what):
    from fedlesscan_amd import MXLayer
    assert isinstance(got, MXLayer) and got.q.dtype == FMTS[fmt] and got.e.dtype == torch.float8_e8m0fnu, what
    q, e = _quantise(v, fmt)
    gq, ge = got.q.view(torch.uint8).cpu().numpy().reshape(-1), got.e.view(torch.uint8).cpu().numpy()
    assert gq.shape == q.shape and ge.shape == e.shape, what
    bad = np.flatnonzero(ge != e)
    assert bad.size == 0, f"{what}: {bad.size} scale bytes differ, first {bad[:4]}: {ge[bad[:4]]} != {e[bad[:4]]}"
    bad = np.flatnonzero(gq != q)
    assert bad.size == 0, f"{what}: {bad.size} code bytes differ, first {bad[:4]}: {gq[bad[:4]]} != {q[bad[:4]]}"


# ---------------------------------------------------------------------------
# 1. every input scale byte times every element code: amax, saturation, RNE,
#    F's subnormals, E = 0, float32-subnormal quotients, signed zeros
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["stacked", "table_odd_row"])
@pytest.mark.parametrize("out", list(FMTS))
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_conversion_sweep(dev, fmt, out, layout):
    P = 255 * 256
    codes = (np.arange(P) % 256).astype(np.uint8)
    codes[(codes & 0x7F) == 0x7F if fmt == "e4m3" else (codes & 0x7C) == 0x7C] = 0
    q, E = codes[None], (np.arange(P // 32) // 8).astype(np.uint8)[None]
    v = M._oracle(fmt, q, E, [1], None, None)[0]
    assert np.unique(v[np.isfinite(v)]).size > 1000 and (~np.isfinite(v)).any()
    _same_mx(M._fold(fmt, q, E, layout, dev, [1], out_format=FMTS[out]), v, out, f"{fmt} -> {out}")


# ---------------------------------------------------------------------------
# 2. fold parity over rows, columns, layouts and factor kinds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("stall", [False, True])
@pytest.mark.parametrize("P", [30, T + 96 + 6])
@pytest.mark.parametrize("N", [1, 3, "ahead + 2"])
@pytest.mark.parametrize("fmt, out", [("e4m3", "e2m1"), ("e2m1", "e4m3"), ("e5m2", "e5m2")])
def test_fold_parity(dev, fmt, out, N, P, stall, layout):
    N = M.AHEAD[fmt] + 2 if isinstance(N, str) else N
    exp = M._expect(fmt, N, P, stall, stall)
    w, sc, scales = M._factors(N, stall, stall)
    f32 = torch.zeros(P + 4, dtype=torch.float32, device=dev)
    got = M._fold(fmt, *M._bytes(fmt, N, P), layout, dev, w, sc, scales=scales, out_format=FMTS[out], out=f32[:P])
    _same_mx(got, exp[0], out, "MX result")
    M._same(f32[:P], exp, "out=")
    assert not f32[P:].any()


# ---------------------------------------------------------------------------
# 3. fp8 rows: a block is two lanes' units, or one lane's at the row's end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["stacked", "table", "table_odd_row"])
@pytest.mark.parametrize("P", [48, 70, _lib.FA_FP8_TILE_COLS + 16 + 7])
@pytest.mark.parametrize("out", ["e4m3", "e2m1"])
def test_fp8_source(dev, out, P, layout):
    P, N = P - (P % 2 if out == "e2m1" else 0), 3
    w, sc, scales = F8._factors(N, False, True)
    b = F8._bytes("e5m2", N, P)
    exp = F8._oracle("e5m2", b, w, sc, scales)
    f32 = torch.zeros(P, dtype=torch.float32, device=dev)
    got = F8._fold(F8._rows(b, "e5m2", layout, dev), w, sc, scales=scales, out_format=FMTS[out], out=f32)
    _same_mx(got, exp[0], out, "MX result")
    F8._same(f32, exp, "out=")


# ---------------------------------------------------------------------------
# 4. edge blocks: e5m2 rows whose halved sums are the quotients named below
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("out", list(FMTS))
def test_edge_blocks(dev, out):
    emax, maxnorm = QF[out]
    top, k = (0x3E if out == "e2m1" else 0x3F), 3  # 1.5 or 1.75: maxnorm's significand; blocks scaled by 2^k
    # (row 0's code at column 5 and its scale byte, row 1's): quotient = (x0 + x1) / 2
    blocks = [(0x7F, 127, 0, 127), (0x7C, 127, 0, 127),                       # a NaN; +inf
              (0, 127, 0, 127), (0x80, 127, 0x80, 127),                       # zeros; -0 (filled below)
              (top, 128 + emax + k, 0, 127),                                  # amax = maxnorm * 2^k
              (top, 128 + emax + k, 0x3C, 128 + emax + k - 23),               # ... and its next float32 up
              (0x3C, 128 + k, 0, 127), (0x3C, 128 + k, 0xBC, 128 + k - 24),   # amax = 2^k; its next float32 down
              (0x7F, 127, 0, 127)]                                            # the last, partial block: a NaN
    P = 32 * (len(blocks) - 1) + 8
    q, E = np.zeros((2, 32 * len(blocks)), dtype=np.uint8), np.zeros((2, len(blocks)), dtype=np.uint8)
    for b, (c0, e0, c1, e1) in enumerate(blocks):
        if b not in (2, 3):
            q[0, 32 * b:32 * b + 5] = [0x38, 0xB9, 0x01, 0x80, 0x35]  # smaller neighbours: .5, -.625, 2^-16, -0, .3125
        q[:, 32 * b:32 * b + 32] |= 0x80 if b == 3 else 0
        q[0, 32 * b + 5], q[1, 32 * b + 5], E[0, b], E[1, b] = c0, c1, e0, e1
    q = q[:, :P]
    v = M._oracle("e5m2", q, E, [1, 1], None, None)[0]
    blk = lambda b: v[32 * b:32 * b + 32]
    assert np.isnan(blk(0)).any() and np.isinf(blk(1)).any() and np.isnan(blk(8)).any() and blk(8).size == 8
    assert not blk(2).any() and not blk(3).any() and np.signbit(blk(3)).all() and not np.signbit(blk(2)).any()
    up, one = np.float32(maxnorm * 2.0 ** k), np.float32(2.0 ** k)
    assert [np.abs(blk(b)).max() for b in (4, 5, 6, 7)] == [up, np.nextafter(up, np.float32(np.inf)), one,
                                                           np.nextafter(one, np.float32(0))]
    for layout in ("stacked", "table_odd_row"):
        _same_mx(M._fold("e5m2", q, E, layout, dev, [1, 1], out_format=FMTS[out]), v, out, layout)


# ---------------------------------------------------------------------------
# 5. closure: the result is a valid MX row of a further fold
# ---------------------------------------------------------------------------
def test_result_folds_as_an_mx_row(dev):
    from fedlesscan_amd import engine
    N, P = 3, T + 96 + 6
    w, sc, scales = M._factors(N, True, True)
    buf = (torch.zeros(P // 2, dtype=torch.uint8, device=dev).view(FMTS["e2m1"]),
           torch.zeros((P + 31) // 32, dtype=torch.uint8, device=dev))
    got = M._fold("e4m3", *M._bytes("e4m3", N, P), "stacked", dev, w, sc, scales=scales, out_mx=buf)
    assert got.q.data_ptr() == buf[0].data_ptr() and got.e.data_ptr() == buf[1].data_ptr()
    q, e = got.q.view(torch.uint8).cpu().numpy()[None], got.e.view(torch.uint8).cpu().numpy()[None]
    again = engine.fold_stacked(got.q.reshape(1, -1), [1], block_scales=got.e.reshape(1, -1))
    M._same(again, M._oracle("e2m1", q, e, [1], None, None), "second level")


# ---------------------------------------------------------------------------
# 6. aggregate_layers(out_format=...) and the refusals
# ---------------------------------------------------------------------------
def test_aggregate_layers_returns_mx_layers(dev):
    from fedlesscan_amd import InvalidParameterShapeError, MXLayer, engine
    layers, n = [("e4m3", (2, 3, 4, 8)), ("e5m2", (7, 10))], 3
    w, _, _ = M._factors(n, False, False)
    data = [M._bytes(fmt, n, int(np.prod(shp))) for fmt, shp in layers]
    params = [[MXLayer(torch.from_numpy(np.array(q[i])).to(dev).view(FMTS[fmt]).reshape(shp),
                       torch.from_numpy(np.array(E[i])).to(dev)) for (fmt, shp), (q, E) in zip(layers, data)]
              for i in range(n)]
    for out, last in (("e2m1", 2), ("e5m2", 1)):
        before = engine.stats["mx_out_folds"]
        outs = engine.aggregate_layers(params, w, out_format=FMTS[out])
        assert engine.stats["mx_out_folds"] == before + len(layers)
        for (fmt, shp), (q, E), o in zip(layers, data, outs):
            assert tuple(o.q.shape) == shp[:-1] + (shp[-1] // last,) and tuple(o.e.shape) == ((q.shape[1] + 31) // 32,)
            _same_mx(o, M._oracle(fmt, q, E, w, None, None)[0], out, f"{fmt} {shp} -> {out}")
    q, E = (torch.from_numpy(np.array(b)).to(dev) for b in data[1])
    X = q.view(FMTS["e5m2"])
    with pytest.raises(InvalidParameterShapeError, match="want_bf16"):
        engine.fold_stacked(X, w, block_scales=E, out_format=FMTS["e4m3"], want_bf16=True)
    with pytest.raises(InvalidParameterShapeError, match="fp8 and MX rows"):
        engine.fold_stacked(torch.ones((3, 70), device=dev), w, out_format=FMTS["e4m3"])
    with pytest.raises(InvalidParameterShapeError, match="two columns per byte"):
        engine.fold_stacked(X[:, :33], w, block_scales=E[:, :2], out_format=FMTS["e2m1"])
    with pytest.raises(InvalidParameterShapeError, match="device fp8 and MX layers"):
        engine.aggregate_layers([[torch.ones(4, device=dev)]] * 3, w, out_format=FMTS["e4m3"])
