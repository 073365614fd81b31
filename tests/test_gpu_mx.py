"""GPU parity of the MX folds (fa_fedavg_mx, fa_fedavg_mx_ptrs) through
engine.fold_stacked, engine.fold_rows and the strategy classes.

The specification is the upcast on the CPU: the committed float32 oracle over
upcast(q) * E.view(float8_e8m0fnu).to(float32).repeat_interleave(32)[:P]
[* np.float32(scale)], formed in numpy float32 (e2m1 through a 16-entry table).
Results are compared as uint32 bit patterns (NaN positions by isnan); no tolerance.
"""
import functools

import numpy as np
import pytest

from fedlesscan_amd import _lib, synth
from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = _lib.FA_MX_TILE_COLS
FMTS = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2, "e2m1": torch.float4_e2m1fn_x2}
AHEAD = {"e4m3": _lib.FA_MX_ROWS_AHEAD_FP8, "e5m2": _lib.FA_MX_ROWS_AHEAD_FP8, "e2m1": _lib.FA_MX_ROWS_AHEAD_FP4}
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=np.float32)
LAYOUTS = ["stacked", "pitched", "table", "table_odd_row"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _oracle(fmt, q, E, w, sc, scales, total=None):
    """(float32 result, its RNE bf16 bits) of the float32 oracle over the rows dequantised on the CPU.
    q: [N, row bytes] element bytes, E: [N, ceil(P / 32)] scale bytes; total: the divisor where it is not sum(w)."""
    if fmt == "e2m1":
        X = np.stack([E2M1[q & 15], E2M1[q >> 4]], axis=-1).reshape(q.shape[0], -1)
    else:
        X = torch.from_numpy(np.array(q)).view(FMTS[fmt]).to(torch.float32).numpy()
    S = torch.from_numpy(np.array(E)).view(torch.float8_e8m0fnu).to(torch.float32).numpy()
    with np.errstate(all="ignore"):
        X = X * np.repeat(S, 32, axis=1)[:, :X.shape[1]]
        if scales is not None:
            X = X * np.array([np.float32(c) for c in scales], dtype=np.float32)[:, None]
        assert X.dtype == np.float32
        e = O.fedavg_stacked(X, w, sc, total=total)
    assert e.dtype == np.float32
    return e, synth.f32_to_bf16_bits(e)


@functools.lru_cache(maxsize=None)
def _bytes(fmt: str, N: int, P: int):
    """Uniform element codes (the format's NaN / Inf codes zeroed) and scale bytes in 117..137."""
    rng = np.random.default_rng(1000 * N + P)
    q = rng.integers(0, 256, size=(N, P // 2 if fmt == "e2m1" else P), dtype=np.uint8)
    if fmt != "e2m1":
        q[(q & 0x7F) == 0x7F if fmt == "e4m3" else (q & 0x7C) == 0x7C] = 0
    E = rng.integers(117, 138, size=(N, (P + 31) // 32), dtype=np.uint8)
    q.setflags(write=False), E.setflags(write=False)
    return q, E


def _factors(N, scored, scaled):
    w = synth.cardinalities(7, N)
    sc = [(r + 1) / 11 for r in synth.round_ids(7, N, 10, 2)] if scored else None
    scales = [float(x) for x in np.random.default_rng(N).uniform(0.01, 2.0, N)] if scaled else None
    return w, sc, scales


@functools.lru_cache(maxsize=None)
def _expect(fmt, N, P, scored, scaled):
    return _oracle(fmt, *_bytes(fmt, N, P), *_factors(N, scored, scaled))


def _place(b: np.ndarray, layout, dev, dtype, align):
    """The byte rows b on the device as dtype: a stacked matrix (tight, or at a
    pitch above the row), or a list of separately placed rows (at `align`
    bytes, or the middle one a byte off)."""
    N, n = b.shape
    if layout in ("stacked", "pitched"):
        ld = n if layout == "stacked" else (n + 15) // 16 * 16 + align
        buf = torch.zeros((N, ld), dtype=torch.uint8, device=dev)
        buf[:, :n] = torch.from_numpy(np.array(b)).to(dev)
        return buf.view(dtype)[:, :n]
    rows = []
    for i in range(N):
        off = 1 if (layout == "table_odd_row" and i == N // 2) else 0
        buf = torch.zeros(n + 48 + 16 * (i % 3), dtype=torch.uint8, device=dev)  # never a constant stride
        buf[off:off + n] = torch.from_numpy(np.array(b[i])).to(dev)
        rows.append(buf[off:off + n].view(dtype))
    return rows


def _fold(fmt, q, E, layout, dev, *args, **kw):
    """Data rows 16-B aligned unless the layout says otherwise; scale rows at pitch + 3 / one byte off."""
    from fedlesscan_amd import engine
    rows = _place(q, layout, dev, FMTS[fmt], 16)
    es = _place(E, "table_odd_row" if layout.startswith("table") else layout, dev, torch.float8_e8m0fnu, 3)
    return (engine.fold_rows if isinstance(rows, list) else engine.fold_stacked)(rows, *args, block_scales=es, **kw)


def _same(got, exp, what):
    """got: a float32 or bfloat16 CUDA tensor; exp: (float32, bf16 bits)."""
    if got.dtype == torch.bfloat16:
        g = got.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << 16
        e = exp[1].astype(np.uint32) << 16
    else:
        assert got.dtype == torch.float32
        g, e = got.cpu().numpy().view(np.uint32), exp[0].view(np.uint32)
    assert g.shape == e.shape, what
    gn, en = np.isnan(g.view(np.float32)), np.isnan(e.view(np.float32))
    assert np.array_equal(gn, en), f"{what}: NaN positions"
    bad = np.flatnonzero((g != e) & ~en)
    assert bad.size == 0, f"{what}: {bad.size} columns differ, first {bad[:4]}: {g[bad[:4]]} != {e[bad[:4]]}"


# ---------------------------------------------------------------------------
# 1. every scale byte times every element code: the conversion and the scaling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["stacked", "table", "table_odd_row"])
@pytest.mark.parametrize("w, scales", [([1], None), ([1, 2, 0], None), ([1, 2, 0], [0.25, 1.7, 3.0])])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_every_scale_byte_times_every_code(dev, fmt, w, scales, layout):
    N, fp4 = len(w), fmt == "e2m1"
    P = 256 * (32 if fp4 else 256)  # block b carries scale byte b // k: 1 (fp4) or 8 (fp8) blocks per byte
    codes = np.arange(P, dtype=np.int64) % (16 if fp4 else 256)
    row = (codes[0::2] | codes[1::2] << 4 if fp4 else codes).astype(np.uint8)
    scale_row = (np.arange(P // 32) // (1 if fp4 else 8)).astype(np.uint8)
    q = np.stack([np.roll(row, 85 * i) for i in range(N)])
    E = np.stack([np.roll(scale_row, 3 * i) for i in range(N)])
    exp = _oracle(fmt, q, E, w, None, scales)
    # the reference is NaN only where the format says so (one row: its NaN codes under the 255 scale bytes
    # below 255, and every element under e = 255) and finite on most of the rest, subnormals included
    finite = np.isfinite(exp[0])
    if N == 1:
        assert np.isnan(exp[0]).sum() == {"e4m3": 2, "e5m2": 6, "e2m1": 0}[fmt] * 255 + (32 if fp4 else 256)
    assert (~finite).sum() < P // 4 and np.unique(exp[0][finite]).size > 1000
    _same(_fold(fmt, q, E, layout, dev, w, scales=scales), exp, "float32")
    _same(_fold(fmt, q, E, layout, dev, w, scales=scales, want_bf16=True)[1], exp, "bf16")


# ---------------------------------------------------------------------------
# 2. shape edges: columns around a block and a tile, rows around the row group
# ---------------------------------------------------------------------------
def _shapes(fmt):
    U = AHEAD[fmt]
    Ns = [1, 2, U - 1, U, U + 1, 2 * U + 1, 33]
    Ps = [2, 30, 32, 34, 62, T - 2, T, T + 2, 2 * T + 32 + 6] + ([] if fmt == "e2m1" else [1, 15, 17, 33])
    return [(fmt, Ns[k % len(Ns)], P) for k, P in enumerate(Ps)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("fmt, N, P", [c for f in FMTS for c in _shapes(f)])
def test_shape_edges(dev, fmt, N, P, scored, scaled, layout):
    exp = _expect(fmt, N, P, scored, scaled)
    assert np.isfinite(exp[0]).all() and (exp[0] != 0).any()
    w, sc, scales = _factors(N, scored, scaled)
    q, E = _bytes(fmt, N, P)
    _same(_fold(fmt, q, E, layout, dev, w, sc, scales=scales), exp, "float32 alone")
    ob = torch.zeros(P + 8, dtype=torch.bfloat16, device=dev)
    got = _fold(fmt, q, E, layout, dev, w, sc, scales=scales, out_bf16=ob[:P])
    assert got.data_ptr() == ob.data_ptr() and not ob[P:].any()
    _same(got, exp, "bf16 alone")
    f, h = _fold(fmt, q, E, layout, dev, w, sc, scales=scales, want_bf16=True)
    _same(f, exp, "float32 of both")
    _same(h, exp, "bf16 of both")


# ---------------------------------------------------------------------------
# 3. several tiles per block of the grid-stride walk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["pitched", "table"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_several_tiles_per_block(dev, fmt, layout):
    N, P = 3, 3 * torch.cuda.get_device_properties(dev).multi_processor_count * T + 38
    w, sc, scales = _factors(N, True, True)
    _same(_fold(fmt, *_bytes(fmt, N, P), layout, dev, w, sc, scales=scales), _expect(fmt, N, P, True, True), layout)


# ---------------------------------------------------------------------------
# 4. the public interface
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("stall_aware", [False, True])
def test_strategy_classes_fold_mx_models(dev, stall_aware):
    from fedlesscan_amd import FedAvgAggregator, MXLayer, StallAwareAggregator, engine
    # (format, logical shape, per-client scales?): fp4; fp8 with a scale; a size that is no multiple of 32
    layers, n = [("e2m1", (25, 64), False), ("e4m3", (50, 1024), True), ("e5m2", (7, 9), False)], 5
    w, _, _ = _factors(n, False, False)
    feats = [{"round_id": r} for r in synth.round_ids(7, n, 10, 2)]
    sc = O.score_clients(feats, 10) if stall_aware else None
    data = [_bytes(fmt, n + li, int(np.prod(shp))) for li, (fmt, shp, _) in enumerate(layers)]
    scales = [[0.5 + 0.37 * i + 0.11 * li for i in range(n)] if c else None for li, (_, _, c) in enumerate(layers)]

    def layer(i, li):
        fmt, shp, _ = layers[li]
        q, E = data[li]
        qshape = shp[:-1] + (shp[-1] // 2,) if fmt == "e2m1" else shp
        return MXLayer(torch.from_numpy(np.array(q[i])).to(dev).view(FMTS[fmt]).reshape(qshape),
                       torch.from_numpy(np.array(E[i])).to(dev), scales[li] and scales[li][i])

    params = [[layer(i, li) for li in range(len(layers))] for i in range(n)]
    before = engine.stats["mx_folds"]
    if stall_aware:
        outs = StallAwareAggregator(10, None)._aggregate(feats, params, w)
    else:
        outs = FedAvgAggregator()._aggregate(params, w)
    assert engine.stats["mx_folds"] == before + len(layers)
    for li, (fmt, shp, _) in enumerate(layers):
        q, E = data[li]
        assert tuple(outs[li].shape) == shp
        _same(outs[li].reshape(-1), _oracle(fmt, q[:n], E[:n], w, sc, scales[li]), f"layer {li}")


def test_refusals_answer_on_the_host(dev):
    from fedlesscan_amd import InvalidParameterShapeError, MXLayer, engine
    q, E = (torch.from_numpy(np.array(b)).to(dev) for b in _bytes("e5m2", 2, 64))
    with pytest.raises(InvalidParameterShapeError, match="block_scales"):
        engine.fold_stacked(torch.ones((2, 64), device=dev), [1, 2], block_scales=E)
    with pytest.raises(InvalidParameterShapeError, match="block_scales"):
        engine.fold_stacked(q.view(torch.float8_e5m2), [1, 2], block_scales=E.float())
    with pytest.raises(InvalidParameterShapeError, match="scale bytes"):  # a short scale row
        engine.fold_rows([q[0].view(torch.float8_e5m2), q[1].clone().view(torch.float8_e5m2)], [1, 2],
                         block_scales=[E[0], E[1, :1]])
    mixed = [[MXLayer(q[0].view(torch.float8_e5m2), E[0])], [MXLayer(q[1].view(torch.float8_e4m3fn), E[1])]]
    with pytest.raises(InvalidParameterShapeError, match="one format"):
        engine.aggregate_layers(mixed, [1, 2])
    with pytest.raises(InvalidParameterShapeError, match="MXLayer or none"):
        engine.aggregate_layers([mixed[0], [q[1].view(torch.float8_e5m2)]], [1, 2])
