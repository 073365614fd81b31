"""GPU parity of the MX layer tables (fa_fedavg_mx_layers, fa_fedavg_mx_q_layers)
through engine.ModelRowSet / fold_model_rows, engine.aggregate_layers, the
strategy classes and the bench library's capped-grid entries.

Per layer the specification is test_gpu_mx.py's: the committed float32 oracle
over the rows dequantised on the CPU, and test_gpu_mx_out.py's _quantise of its
quotients.  Bit patterns and bytes are compared; no tolerance.
"""
import functools

import numpy as np
import pytest

import test_gpu_mx as M
import test_gpu_mx_out as MQ
from fedlesscan_amd import _lib, synth
from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W = _lib.FA_MX_WAVE_TILE_COLS
# a lone partial block; exactly one wave tile; two columns; more than one workgroup with a partial last block
# (the unaligned layer); exactly two blocks; one wave tile plus one block
SIZES = [30, W, 2, 5 * W + 96 + 6, 64, W + 32]
ODD = 3  # the layer whose middle client row is one byte off: the one-column path between aligned layers
FMTS = M.FMTS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _scales(N, k):
    return [c * (1 + k / 8) for c in M._factors(N, False, True)[2]]


@functools.lru_cache(maxsize=None)
def _expect(fmt, N, scored, scaled):
    """Per layer: (float32 result, its bf16 bits) of the oracle over that layer alone."""
    w, sc, _ = M._factors(N, scored, False)
    return [M._oracle(fmt, *M._bytes(fmt, N, P), w, sc, _scales(N, k) if scaled else None) for k, P in enumerate(SIZES)]


def _model(fmt, N, dev, scaled=False):
    """N clients x len(SIZES) MXLayers: rows separately allocated, never at a constant stride, the middle
    scale row of every layer (and the middle data row of layer ODD) a byte off."""
    from fedlesscan_amd import MXLayer
    cols = []
    for k, P in enumerate(SIZES):
        q, E = M._bytes(fmt, N, P)
        rows = M._place(q, "table_odd_row" if k == ODD else "table", dev, FMTS[fmt], 16)
        es = M._place(E, "table_odd_row", dev, torch.float8_e8m0fnu, 3)
        cs = _scales(N, k) if (scaled if isinstance(scaled, bool) else scaled[k]) else [None] * N
        cols.append([MXLayer(r, e, c) for r, e, c in zip(rows, es, cs)])
    return [[col[i] for col in cols] for i in range(N)]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("N", [1, 3, "ahead + 2"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_fold_parity(dev, fmt, N, scored, scaled):
    from fedlesscan_amd import engine
    N = M.AHEAD[fmt] + 2 if isinstance(N, str) else N
    exp = _expect(fmt, N, scored, scaled)
    w, sc, _ = M._factors(N, scored, False)
    ms = engine.ModelRowSet(_model(fmt, N, dev, scaled))
    assert ms.host_plan[:, 3].tolist() == [int(k != ODD) for k in range(len(SIZES))] and ms.tiles == 168
    before = dict(engine.stats)
    got = engine.fold_model_rows(ms, w, sc)
    assert engine.stats["mx_table_folds"] == before["mx_table_folds"] + 1
    assert engine.stats["mx_folds"] == before["mx_folds"] + len(SIZES)
    for k, P in enumerate(SIZES):
        assert tuple(got[k].shape) == (P,)
        M._same(got[k], exp[k], f"layer {k}")
    if fmt == "e5m2":
        ob = torch.zeros(ms.elems, dtype=torch.bfloat16, device=dev)
        f, h = engine.fold_model_rows(ms, w, sc, want_bf16=True, out_bf16=ob)
        for k, P in enumerate(SIZES):
            M._same(f[k], exp[k], f"float32 of both, layer {k}")
            M._same(h[k], exp[k], f"bf16, layer {k}")
            o = ms.offsets[k]
            assert h[k].data_ptr() == ob.data_ptr() + 2 * o and not ob[o + P:o + (P + 63) // 64 * 64].any()


@pytest.mark.parametrize("fmt, out, with_out", [("e4m3", "e2m1", True), ("e2m1", "e4m3", False), ("e5m2", "e5m2", False)])
def test_mx_output_and_second_level(dev, fmt, out, with_out):
    from fedlesscan_amd import engine
    N = 3
    exp = _expect(fmt, N, True, True)
    w, sc, _ = M._factors(N, True, False)
    ms = engine.ModelRowSet(_model(fmt, N, dev, True))
    f32 = torch.zeros(ms.elems, dtype=torch.float32, device=dev) if with_out else None
    before = engine.stats["mx_out_folds"]
    got = engine.fold_model_rows(ms, w, sc, out_format=FMTS[out], out=f32)
    assert engine.stats["mx_out_folds"] == before + len(SIZES)
    for k, (P, o) in enumerate(zip(SIZES, ms.offsets)):
        MQ._same_mx(got[k], exp[k][0], out, f"layer {k}")
        if with_out:  # the float32 result beside it, nothing written behind the layer
            M._same(f32[o:o + P], exp[k], f"out=, layer {k}")
            assert not f32[o + P:o + (P + 63) // 64 * 64].any()
    # the returned layers are one client of a second-level model
    again = engine.fold_model_rows([got], [1])
    for k in range(len(SIZES)):
        q, e = (t.view(torch.uint8).cpu().numpy().reshape(1, -1) for t in got[k][:2])
        M._same(again[k].reshape(-1), M._oracle(out, q, e, [1], None, None), f"second level, layer {k}")


@pytest.mark.parametrize("fmt, out", [("e2m1", None), ("e4m3", "e5m2")])
def test_capped_grid_walks_every_wave_through_several_layers(dev, fmt, out):
    from fedlesscan_amd import MXLayer, engine
    N, B = 3, _lib.load_bench()
    exp = _expect(fmt, N, False, False)
    w, _, _ = M._factors(N, False, False)
    ms = engine.ModelRowSet(_model(fmt, N, dev))
    assert ms.tiles > 3 * 4 * len(SIZES)  # 3 blocks of 4 waves: every wave takes 14 wave tiles
    a = torch.tensor(np.array(w, dtype=np.float32), device=dev)
    f32 = torch.zeros(ms.elems, dtype=torch.float32, device=dev)
    args = [_lib.FA_MX_E2M1 if fmt == "e2m1" else _lib.FA_MX_E4M3, ms.ptrs.data_ptr(), ms.scale_ptrs.data_ptr(),
            ms.plan.data_ptr(), ms.L, N, ms.tiles, a.data_ptr(), None, None, float(np.float32(sum(w))), f32.data_ptr()]
    st = engine.stream_ptr(dev)
    if out is None:
        _lib.check(B.fa_fedavg_mx_layers_form(*args, None, st, 3), "fa_fedavg_mx_layers_form", bench=True)
    else:
        qf = torch.zeros(ms.elems, dtype=torch.uint8, device=dev)
        ef = torch.zeros(ms.elems // 32, dtype=torch.uint8, device=dev)
        _lib.check(B.fa_fedavg_mx_q_layers_form(*args, _lib.FA_MX_E5M2, qf.data_ptr(), ef.data_ptr(), st, 3),
                   "fa_fedavg_mx_q_layers_form", bench=True)
    for k, (P, o) in enumerate(zip(SIZES, ms.offsets)):
        M._same(f32[o:o + P], exp[k], f"layer {k}")
        if out is not None:
            layer = MXLayer(qf[o:o + P].view(FMTS[out]), ef[o // 32:o // 32 + (P + 31) // 32].view(torch.float8_e8m0fnu))
            MQ._same_mx(layer, exp[k][0], out, f"layer {k}")


def test_prepared_set_is_refolded_after_contents_and_scales_change(dev):
    from fedlesscan_amd import engine
    fmt, N = "e2m1", 3
    w, sc, _ = M._factors(N, True, False)
    params = _model(fmt, N, dev, True)
    ms = engine.ModelRowSet(params)
    for k in range(len(SIZES)):
        M._same(engine.fold_model_rows(ms, w, sc)[k], _expect(fmt, N, True, True)[k], f"first fold, layer {k}")
    for k in range(len(SIZES)):  # client i now holds what client i + 1 held
        for t in ("q", "e"):
            rows = [getattr(params[i][k], t).view(torch.uint8) for i in range(N)]
            for r, old in zip(rows, [rows[(i + 1) % N].clone() for i in range(N)]):
                r.copy_(old)
    scales = [[0.3 + 0.2 * i + 0.05 * k for i in range(N)] for k in range(len(SIZES))]
    got = engine.fold_model_rows(ms, w, sc, scales=scales)
    for k, P in enumerate(SIZES):
        q, E = (np.roll(b, -1, axis=0) for b in M._bytes(fmt, N, P))
        M._same(got[k], M._oracle(fmt, q, E, w, sc, scales[k]), f"refold, layer {k}")


@pytest.mark.parametrize("route", ["aggregate_layers", "FedAvgAggregator", "StallAwareAggregator"])
def test_public_routes_take_one_launch_per_sub_group(dev, route, monkeypatch):
    from fedlesscan_amd import FedAvgAggregator, StallAwareAggregator, engine
    N = 5
    w, _, _ = M._factors(N, False, False)
    feats = [{"round_id": r} for r in synth.round_ids(7, N, 10, 2)]
    params = _model("e4m3", N, dev, [k >= 3 for k in range(len(SIZES))])  # two sub-groups: three layers each

    def fold():
        if route == "aggregate_layers":
            return engine.aggregate_layers(params, w)
        if route == "FedAvgAggregator":
            return FedAvgAggregator()._aggregate(params, w)
        return StallAwareAggregator(10, None)._aggregate(feats, params, w)

    before = dict(engine.stats)
    got = fold()
    assert engine.stats["mx_table_folds"] == before["mx_table_folds"] + 2
    assert engine.stats["mx_folds"] == before["mx_folds"] + len(SIZES)
    monkeypatch.setenv("FEDAVG_LAYER_TABLE", "0")
    per_layer = fold()
    assert engine.stats["mx_table_folds"] == before["mx_table_folds"] + 2
    assert engine.stats["mx_folds"] == before["mx_folds"] + 2 * len(SIZES)
    sc = O.score_clients(feats, 10) if route == "StallAwareAggregator" else None
    for k, P in enumerate(SIZES):
        assert torch.equal(got[k].view(torch.int32), per_layer[k].view(torch.int32)), f"layer {k}"
        q, E = M._bytes("e4m3", N, P)
        M._same(got[k], M._oracle("e4m3", q, E, w, sc, _scales(N, k) if k >= 3 else None), f"layer {k}")


def test_refusals_answer_on_the_host(dev):
    from fedlesscan_amd import InvalidParameterShapeError, MXLayer, engine
    one = lambda fmt, P, c=None: [MXLayer(torch.zeros(P, dtype=torch.uint8, device=dev).view(FMTS[fmt]),
                                          torch.zeros((P + 31) // 32, dtype=torch.uint8, device=dev), c)]
    with pytest.raises(InvalidParameterShapeError, match="one format"):
        engine.ModelRowSet([one("e4m3", 64) + one("e5m2", 64)] * 2)
    with pytest.raises(InvalidParameterShapeError, match="all layers carry client scales or none"):
        engine.ModelRowSet([one("e4m3", 64, 0.5) + one("e4m3", 64)] * 2)
    ms = engine.ModelRowSet([one("e4m3", 64) + one("e4m3", 31)] * 2)
    before = engine.stats["mx_table_folds"]
    with pytest.raises(InvalidParameterShapeError, match="two columns per byte"):
        engine.fold_model_rows(ms, [1, 2], out_format=FMTS["e2m1"])
    with pytest.raises(InvalidParameterShapeError, match="want_bf16"):
        engine.fold_model_rows(ms, [1, 2], out_format=FMTS["e4m3"], want_bf16=True)
    assert engine.stats["mx_table_folds"] == before
