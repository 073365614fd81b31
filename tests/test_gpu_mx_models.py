"""Mixed models through the host routes of the fp8 / MX family: one interleaved
model (fp32, bf16 and integer layers, MX layers of three formats with and
without client scales, N-dimensional, 0-dim and zero-size ones, a ScaledLayer
and a plain fp8 layer) through aggregate_layers and the strategy classes, with
zip() truncation, with out_format=, and fold_model_rows' outputs when the
caller's buffers cannot be used as given.  Every layer is checked against the
oracle of that layer alone: bit patterns and bytes, no tolerance.
"""
import numpy as np
import pytest

import test_gpu_fp8 as F8
import test_gpu_mx as M
import test_gpu_mx_out as MQ
from fedlesscan_amd import synth
from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMTS = M.FMTS
N = 5
# (kind, shape as the client gives it): "mx_<fmt>" / "mx_<fmt>+c" (client scales), "scaled" (ScaledLayer e4m3fn),
# "fp8" (plain e4m3fn), or a torch dtype name
MODEL = [("float32", (10,)), ("mx_e4m3", (3, 4, 8)), ("int64", ()), ("mx_e4m3+c", (6, 16)), ("scaled", (5, 7)),
         ("fp8", (9,)), ("mx_e2m1", (4, 8)), ("mx_e2m1", (2, 3, 4)), ("bfloat16", (3, 5)), ("mx_e4m3", (40,)),
         ("mx_e5m2", ()), ("mx_e4m3", (0,))]
ROUTES = ["aggregate_layers", "FedAvgAggregator", "StallAwareAggregator"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _size(shape):
    return int(np.prod(shape)) if len(shape) else 1


def _host_model(n):
    """Per layer: the n clients' host data -- (q, E, scales) byte rows of an MX / fp8 layer, or an [n, size] array."""
    data = []
    for li, (kind, shape) in enumerate(MODEL):
        size = _size(shape)
        cs = [0.5 + 0.37 * i + 0.11 * li for i in range(n)]
        if kind.startswith("mx_"):
            fmt = kind[3:7]
            q, E = M._bytes(fmt, n + li, 2 * size if fmt == "e2m1" else size) if size else (
                np.zeros((n, 0), np.uint8), np.zeros((n, 0), np.uint8))
            data.append((q[:n], E[:n], cs if kind.endswith("+c") else None))
        elif kind in ("scaled", "fp8"):
            data.append((F8._bytes("e4m3fn", n + li, size)[:n], None, cs if kind == "scaled" else None))
        elif kind == "int64":
            data.append(np.arange(3, 3 + n, dtype=np.int64).reshape(n, 1) * 7)
        else:
            x = synth.clients_f32(li, n, 0, size)
            data.append(synth.f32_to_bf16_bits(x) if kind == "bfloat16" else x)
    return data


def _device_model(data, n, dev, kinds=None):
    from fedlesscan_amd import MXLayer, engine
    params = []
    for i in range(n):
        layers = []
        for (kind, shape), d in zip(MODEL, data):
            if kinds is not None and not kinds(kind):
                continue
            if kind.startswith("mx_"):
                q = torch.from_numpy(np.array(d[0][i])).to(dev).view(FMTS[kind[3:7]]).reshape(shape)
                layers.append(MXLayer(q, torch.from_numpy(np.array(d[1][i])).to(dev), d[2] and d[2][i]))
            elif kind in ("scaled", "fp8"):
                q = torch.from_numpy(np.array(d[0][i])).to(dev).view(torch.float8_e4m3fn).reshape(shape)
                layers.append(engine.ScaledLayer(q, d[2][i]) if kind == "scaled" else q)
            elif kind == "bfloat16":
                layers.append(torch.from_numpy(d[i].astype(np.int16)).to(dev).view(torch.bfloat16).reshape(shape))
            else:
                layers.append(torch.from_numpy(np.array(d[i])).to(dev).reshape(shape))
        params.append(layers)
    return params


def _expect(kind, d, n, w, sc, total):
    """(float32 result, bf16 bits) of the oracle over the first n clients of one fp8 / MX layer."""
    if kind.startswith("mx_"):
        return M._oracle(kind[3:7], d[0][:n], d[1][:n], w[:n], sc and sc[:n], d[2] and d[2][:n], total=total)
    return F8._oracle("e4m3fn", d[0][:n], w[:n], sc and sc[:n], d[2] and d[2][:n], total=total)


def _logical(kind, shape):
    return shape[:-1] + (2 * shape[-1],) if kind.startswith("mx_e2m1") and shape else shape


def _fold(route, params, w, feats, **kw):
    from fedlesscan_amd import FedAvgAggregator, StallAwareAggregator, engine
    if route == "aggregate_layers":
        return engine.aggregate_layers(params, w, **kw)
    if route == "FedAvgAggregator":
        return FedAvgAggregator()._aggregate(params, w)
    return StallAwareAggregator(10, None)._aggregate(feats, params, w)


def _check(outs, data, n, w, sc, total):
    assert len(outs) == len(MODEL)
    for li, ((kind, shape), d, got) in enumerate(zip(MODEL, data, outs)):
        what = f"layer {li} ({kind} {shape})"
        if kind.startswith("mx_") or kind in ("scaled", "fp8"):
            assert got.dtype == torch.float32 and tuple(got.shape) == _logical(kind, shape), what
            if kind == "mx_e5m2":  # the 0-dim layer: one column
                assert got.dim() == 0
            M._same(got.reshape(-1), _expect(kind, d, n, w, sc, total), what)
            continue
        # the other dtypes: the literal oracle's own typing of the fold
        X = d[:n] if kind != "bfloat16" else (d[:n].astype(np.uint32) << 16).view(np.float32)
        acc = None
        for i in range(n):  # fedavg_literal / stall_aware_literal on this layer, the divisor the sum of ALL weights
            t = np.multiply(X[i], w[i]) if sc is None else np.multiply(np.multiply(X[i], w[i]), sc[i])
            acc = t if acc is None else np.add(acc, t)
        exp = np.true_divide(acc, sum(w))
        assert tuple(got.shape) == shape and got.cpu().numpy().dtype == exp.dtype, what
        assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint8), exp.reshape(-1).view(np.uint8)), what


@pytest.mark.parametrize("extra", [0, 1])  # one more weight (and score) than clients: zip() truncation
@pytest.mark.parametrize("route", ROUTES)
def test_mixed_model(dev, route, extra, monkeypatch):
    from fedlesscan_amd import engine
    data = _host_model(N)
    params = _device_model(data, N, dev)
    w = synth.cardinalities(7, N + extra)
    feats = [{"round_id": r} for r in synth.round_ids(7, N + extra, 10, 2)]
    sc = O.score_clients(feats, 10) if route == "StallAwareAggregator" else None
    total = sum(w) if extra else None
    keys = ("fp8_folds", "mx_folds", "mx_table_folds", "mx_out_folds")
    before = dict(engine.stats)
    outs = _fold(route, params, w, feats)
    # one table launch per sub-group of two or more MX layers of one format: the three e4m3 layers without
    # client scales (the zero-size one is in the table and is no fold), the two e2m1 layers; a fold of its
    # own for the one e4m3 layer with client scales and the one e5m2 layer; the two fp8 layers per layer
    assert {k: engine.stats[k] - before[k] for k in keys} == {"fp8_folds": 2, "mx_folds": 6, "mx_table_folds": 2,
                                                              "mx_out_folds": 0}
    _check(outs, data, N, w, sc, total)
    monkeypatch.setenv("FEDAVG_LAYER_TABLE", "0")
    before = dict(engine.stats)
    per_layer = _fold(route, params, w, feats)
    assert engine.stats["mx_table_folds"] == before["mx_table_folds"]
    assert engine.stats["mx_folds"] == before["mx_folds"] + 7 and engine.stats["fp8_folds"] == before["fp8_folds"] + 2
    _check(per_layer, data, N, w, sc, total)
    for a, b in zip(outs, per_layer):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("out", list(FMTS))
def test_out_format_on_the_fp8_and_mx_layers(dev, out, extra):
    from fedlesscan_amd import InvalidParameterShapeError, engine
    data = _host_model(N)
    quantised = lambda kind: kind.startswith("mx_") or kind in ("scaled", "fp8")
    odd = lambda kind, shape: _logical(kind, shape)[-1:] in ((7,), (9,)) or not shape  # no pairs of a last dimension
    keep = [li for li, (kind, shape) in enumerate(MODEL) if quantised(kind) and not (out == "e2m1" and odd(kind, shape))]
    w = synth.cardinalities(7, N + extra)
    total = sum(w) if extra else None
    full = _device_model(data, N, dev, quantised)
    if out == "e2m1":
        with pytest.raises(InvalidParameterShapeError, match="float4_e2m1fn_x2 result"):
            engine.aggregate_layers(full, w, out_format=FMTS[out])
        kept = [MODEL[li] for li in keep]
        params = [[x for x, (kind, shape) in zip(p, [m for m in MODEL if quantised(m[0])])
                   if not odd(kind, shape)] for p in full]
        assert len(params[0]) == len(kept)
    else:
        params = full
    before = engine.stats["mx_out_folds"]
    outs = engine.aggregate_layers(params, w, out_format=FMTS[out])
    assert len(outs) == len(keep) and engine.stats["mx_out_folds"] == before + len(keep) - 1  # the zero-size layer
    for li, got in zip(keep, outs):
        kind, shape = MODEL[li]
        shp = _logical(kind, shape)
        what = f"layer {li} ({kind} {shape}) -> {out}"
        assert tuple(got.q.shape) == (shp[:-1] + (shp[-1] // 2,) if out == "e2m1" else shp), what
        assert got.e.numel() == (_size(shp) + 31) // 32 if _size(shp) and shp != (0,) else got.e.numel() == 0, what
        MQ._same_mx(type(got)(got.q.reshape(-1), got.e), _expect(kind, data[li], N, w, None, total)[0], out, what)


def test_fold_model_rows_with_unusable_outputs(dev):
    """out= off 16 bytes, out_bf16= over a client's data row, out_mx= whose scale buffer is client 0's own
    scale row of the last layer, out_mx= longer than needed: what a fresh buffer gives, in the caller's
    buffer, nothing written past the model's extent."""
    from fedlesscan_amd import MXLayer, engine
    fmt, sizes, n = "e4m3", [64, 30, 70], 3
    w, sc, _ = M._factors(n, True, False)
    data = [M._bytes(fmt, n, P) for P in sizes]
    pool = torch.zeros(4096, dtype=torch.uint8, device=dev)  # client 0's rows of the last layer live in here
    cols = []
    for k, (q, E) in enumerate(data):
        rows = M._place(q, "table", dev, FMTS[fmt], 16)
        es = M._place(E, "table", dev, torch.float8_e8m0fnu, 3)
        if k == 2:
            pool[1024:1024 + 70] = torch.from_numpy(np.array(q[0])).to(dev)
            pool[2048:2048 + 3] = torch.from_numpy(np.array(E[0])).to(dev)
            rows[0], es[0] = pool[1024:1024 + 70].view(FMTS[fmt]), pool[2048:2048 + 3].view(torch.float8_e8m0fnu)
        cols.append([MXLayer(r, e) for r, e in zip(rows, es)])
    params = [[col[i] for col in cols] for i in range(n)]
    ms = engine.ModelRowSet(params)
    E_, exp = ms.elems, [M._oracle(fmt, q, E, w, sc, None) for q, E in data]
    fresh = engine.fold_model_rows(ms, w, sc, out_format=FMTS["e5m2"])
    fq, fe = (torch.cat([t.view(torch.uint8).reshape(-1) for t in ts]) for ts in zip(*[(m.q, m.e) for m in fresh]))

    # out= four bytes off a 16-byte boundary
    buf = torch.full((E_ + 9,), 7.0, dtype=torch.float32, device=dev)
    out = buf[1:1 + E_ + 4]
    assert out.data_ptr() % 16 == 4
    got = engine.fold_model_rows(ms, w, sc, out=out)
    for k, (P, o) in enumerate(zip(sizes, ms.offsets)):
        assert got[k].data_ptr() == out.data_ptr() + 4 * o
        M._same(got[k], exp[k], f"out= off 16 bytes, layer {k}")
    assert (buf[:1] == 7).all() and (buf[1 + E_:] == 7).all()

    # out_bf16= over client 0's data row of the last layer: folded from the row's bytes as they were
    ob = pool[1024 - 2 * ms.offsets[2]:].view(torch.bfloat16)[:E_ + 8]
    assert ob.data_ptr() % 16 == 0 and ms.overlaps(ob)
    tail = ob[E_:].clone()
    got = engine.fold_model_rows(ms, w, sc, out_bf16=ob)
    for k, (P, o) in enumerate(zip(sizes, ms.offsets)):
        assert got[k].data_ptr() == ob.data_ptr() + 2 * o
        M._same(got[k], exp[k], f"out_bf16= over a row, layer {k}")
    assert torch.equal(ob[E_:].view(torch.int16), tail.view(torch.int16))
    pool[1024:1024 + 70] = torch.from_numpy(np.array(data[2][0][0])).to(dev)  # the row as it was

    # out_mx= whose scale buffer starts at client 0's scale row of the last layer, both longer than needed
    oq = torch.full((E_ + 16,), 0x55, dtype=torch.uint8, device=dev)
    oe = pool[2048:2048 + E_ // 32 + 5]
    oe[E_ // 32:] = 0x55
    assert ms.overlaps(oe) and not ms.overlaps(oq)
    before = engine.stats["mx_table_folds"]
    got = engine.fold_model_rows(ms, w, sc, out_mx=(oq.view(torch.float8_e5m2), oe.view(torch.float8_e8m0fnu)))
    assert engine.stats["mx_table_folds"] == before + 1
    assert torch.equal(oq[:E_][_mask(ms, sizes, 1, dev)], fq) and (oq[E_:] == 0x55).all()
    assert torch.equal(oe[:E_ // 32][_mask(ms, sizes, 32, dev)], fe) and (oe[E_ // 32:] == 0x55).all()
    for k, P in enumerate(sizes):
        assert got[k].q.data_ptr() == oq.data_ptr() + ms.offsets[k] and got[k].e.data_ptr() == oe.data_ptr() + ms.offsets[k] // 32
        MQ._same_mx(got[k], exp[k][0], "e5m2", f"out_mx= over a scale row, layer {k}")
    pool[2048:2048 + 3] = torch.from_numpy(np.array(data[2][1][0])).to(dev)

    # out_mx= usable as given and longer than needed: folded in place, the rest untouched
    oq, oe = (torch.full((n_ + 16,), 0x55, dtype=torch.uint8, device=dev) for n_ in (E_, E_ // 32))
    got = engine.fold_model_rows(ms, w, sc, out_mx=(oq.view(torch.float8_e5m2), oe.view(torch.float8_e8m0fnu)))
    assert got[0].q.data_ptr() == oq.data_ptr() and (oq[E_:] == 0x55).all() and (oe[E_ // 32:] == 0x55).all()
    for k in range(len(sizes)):
        MQ._same_mx(got[k], exp[k][0], "e5m2", f"out_mx= longer than needed, layer {k}")


def _mask(ms, sizes, per, dev):
    """The positions of a flat result (one per `per` columns) that belong to a layer."""
    m = torch.zeros(ms.elems // per, dtype=torch.bool, device=dev)
    for o, P in zip(ms.offsets, sizes):
        m[o // per:o // per + (P + per - 1) // per] = True
    return m
