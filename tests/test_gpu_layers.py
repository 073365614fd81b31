"""GPU parity of the layer-table folds (fa_fedavg_{f32,bf16,f16,f64}_layers:
every layer of a device-resident model in one launch) and of the routes that
reach them: engine.ModelRowSet / fold_model_rows, aggregate_layers and the
strategy classes.  Every comparison is bit for bit, NaN by position.

Expected values: numpy's literal fold in the layer's own dtype (one multiply,
two with scores, and one add per client, in client order, then a true divide;
bf16 upcast exactly and folded in float32, the bf16 copy its RNE rounding).
Where the factors are Python numbers the same expectation is also checked
against oracle.fedavg_oracle and against engine.fold_rows on that layer alone,
once per shape, where the expectation is made.  Inputs come from
fedlesscan_amd.synth and tests/edge_values.py."""
import numpy as np
import pytest

from fedlesscan_amd import synth
from oracle import fedavg_oracle as O

import edge_values as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F16 = np.float16
KINDS = ["f32", "bf16", "f16", "f64"]
KIDX = {"f32": 0, "bf16": 1, "f16": 2, "f64": 3}  # fa_fedavg_layers_form's dtype
LG = {"f32": 2, "bf16": 3, "f16": 3, "f64": 1}  # columns of a 16-byte unit, as a power of two
FDT = {"f32": np.float32, "bf16": np.float32, "f16": np.float16, "f64": np.float64}  # the factors' dtype
SENT = 0x5A  # a byte no kernel writes keeps this pattern
PAD = 8  # sentinel elements behind every output


def _tdt(kind):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}[kind]


def _rdt(kind):
    return torch.float32 if kind == "bf16" else _tdt(kind)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def parity_cols(kind):
    """In units of the dtype's 16-byte unit count u: four 1-unit tiles and a
    tail, a tail only, nothing, exactly one 1-unit tile, one column, two tiles
    and one unit."""
    u = 1 << LG[kind]
    return [u * 256 * 4 + 13, 5, 0, u * 256, 1, u * 256 * 2 + u]


# ---------------------------------------------------------------------------
# inputs: a layer is an [N, P] host array in the kind's storage type (bf16: the
# uint16 bit patterns), a client's layer its own device allocation
# ---------------------------------------------------------------------------
def _host_layer(kind, seed, N, P):
    X = synth.clients_f32(seed, N, 0, P) if P else np.zeros((N, 0), np.float32)
    if kind == "bf16":
        return synth.f32_to_bf16_bits(X)
    if kind == "f16":
        return X.astype(F16)
    if kind == "f64":
        return X.astype(np.float64) * (1.0 + 1.0 / 3.0)  # mantissas no float32 has
    return X


def _to_dev(kind, row, dev, offset=0):
    """One row as a device tensor of its own; offset: elements past the allocation's start."""
    row = np.ascontiguousarray(row)
    h = row.view(np.int16) if kind == "bf16" else row
    buf = torch.empty(h.size + offset, dtype=torch.int16 if kind == "bf16" else _tdt(kind), device=dev)
    buf[offset:].copy_(torch.from_numpy(h.copy()))
    t = buf[offset:]
    return t.view(torch.bfloat16) if kind == "bf16" else t


def _to_host(kind, t):
    t = t.contiguous().reshape(-1)
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


def _model(kind, dev, seed, N, cols, offsets=None):
    """(host layers, device tensors [layer][client])."""
    host = [_host_layer(kind, seed + 10 * k, N, P) for k, P in enumerate(cols)]
    offsets = offsets or [0] * len(cols)
    tens = [[_to_dev(kind, X[i], dev, off) for i in range(N)] for X, off in zip(host, offsets)]
    for row, off in zip(tens, offsets):
        assert all((t.data_ptr() % 16 == 0) == (off == 0) for t in row if t.numel())
    return host, tens


def _clients(tens):
    """[layer][client] -> the N x L lists the engine takes."""
    return [list(c) for c in zip(*tens)]


def _weights(seed, N):
    return synth.cardinalities(seed, N)  # 1..600: 33 of them sum below 65504, the binary16 divisor stays finite


def _scores(seed, N, R=10):
    return [(r + 1) / (R + 1) for r in synth.round_ids(seed, N, R, 2)]


def _factors(kind, w, sc):
    """Python factors as numpy rounds them for the kind: (a, s or None, divisor)."""
    dt = FDT[kind]
    with np.errstate(all="ignore"):
        return (np.array([dt(v) for v in w], dt), None if sc is None else np.array([dt(v) for v in sc], dt),
                dt(sum(w)))


# ---------------------------------------------------------------------------
# expectations and comparisons
# ---------------------------------------------------------------------------
def _literal(kind, X, a, s, d):
    """numpy's literal fold of one layer.  bf16: (float32, RNE bf16 bits)."""
    if X.shape[1] == 0:
        e = np.zeros(0, np.float32 if kind == "bf16" else X.dtype)
        return (e, np.zeros(0, np.uint16)) if kind == "bf16" else e
    if kind == "bf16":
        X = synth.bf16_bits_to_f32(X)
    dt = X.dtype.type
    with np.errstate(all="ignore"):
        acc = None
        for i in range(X.shape[0]):
            t = np.multiply(X[i], dt(a[i]))
            if s is not None:
                t = np.multiply(t, dt(s[i]))
            acc = t if acc is None else np.add(acc, t)
        out = np.true_divide(acc, dt(d))
    assert out.dtype == X.dtype
    return (out, synth.f32_to_bf16_bits(out)) if kind == "bf16" else out


def _same(a, b) -> bool:
    """Equal bit patterns, NaN by position (floats; uint16: bf16 patterns)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.uint16:
        return E.same_bf16_bits(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~na]))


def _check_layer(kind, got, exp, what):
    """got: host array(s) of one layer -- bf16: (float32 or None, bits or None)."""
    if kind != "bf16":
        assert _same(got, exp), what
        return
    f, b = got
    assert f is not None or b is not None
    if f is not None:
        assert _same(f, exp[0]), what
    if b is not None:
        assert _same(b, exp[1]), what


def _meaningful(kind, exp):
    """Parity is never satisfied by zeros, infinities or NaNs alone."""
    e = np.asarray(exp[0] if kind == "bf16" else exp, dtype=np.float64)
    floor = 2.0 ** -14 if e.size >= 5 else 2.0 ** -24  # a lone column may be small, never zero
    assert e.size == 0 or (np.isfinite(e).all() and (np.abs(e) >= floor).any())


def _engine_layer(kind, t):
    """One layer of an engine result (a tensor, or bf16's (fp32, bf16) pair) on the host, as _check_layer takes it."""
    if kind != "bf16":
        assert t.dtype == _tdt(kind)
        return _to_host(kind, t)
    if isinstance(t, tuple):
        return _to_host(kind, t[0]), _to_host(kind, t[1])
    assert t.dtype == torch.float32
    return _to_host(kind, t), None


_PARITY: dict = {}


def _parity(kind, dev, N, scored):
    """The parity model of (kind, N) on the device and its expectation, made
    once: numpy's literal fold per layer, which is also the oracle's result and
    what fold_rows gives for that layer alone."""
    from fedlesscan_amd import engine
    seed = 100 + N
    mk = (kind, N)
    if mk not in _PARITY:
        _PARITY[mk] = _model(kind, dev, seed, N, parity_cols(kind))
    host, tens = _PARITY[mk]
    key = (kind, N, scored)
    if key not in _PARITY:
        w, sc = _weights(seed, N), (_scores(seed, N) if scored else None)
        exp = []
        for X, rows in zip(host, tens):
            e = _literal(kind, X, *_factors(kind, w, sc))
            _meaningful(kind, e)
            if X.shape[1]:
                with np.errstate(all="ignore"):
                    o = O.fedavg_stacked_bf16(X, w, sc) if kind == "bf16" else O.fedavg_stacked(X, w, sc)
                _check_layer(kind, o, e, ("oracle", key))
                r = engine.fold_rows(rows, w, sc, want_bf16=True) if kind == "bf16" else engine.fold_rows(rows, w, sc)
                _check_layer(kind, _engine_layer(kind, r), e, ("fold_rows", key))
            exp.append(e)
        _PARITY[key] = (w, sc, exp)
    return (host, tens) + _PARITY[key]


# ---------------------------------------------------------------------------
# the raw entry: fa_fedavg_layers_form (units per lane and grid cap given)
# ---------------------------------------------------------------------------
def _raw(kind, dev, tens, units, cap, fac, outs="both"):
    """Plan for `units`, upload table and plan, run the bench-library entry;
    returns the layers on the host after checking that nothing was written
    between the layers or behind the output.  outs (bf16): "f32", "bf16", "both"."""
    from fedlesscan_amd import _lib, engine
    B = _lib.load_bench()
    L, N = len(tens), len(tens[0])
    cols = [row[0].numel() for row in tens]
    aligned = [all(t.data_ptr() % 16 == 0 for t in row) or row[0].numel() == 0 for row in tens]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    plan, tiles, elems, u = engine.layer_plan(cols, aligned, LG[kind], cus, units)
    assert u == units
    ptrs = np.array([[t.data_ptr() for t in row] for row in tens], dtype=np.int64)
    both = torch.from_numpy(np.concatenate([ptrs.reshape(-1), plan.reshape(-1)])).to(dev)
    a, s, d = fac
    da = torch.from_numpy(a.view(np.int16) if kind == "f16" else a).to(dev)
    ds = None if s is None else torch.from_numpy(s.view(np.int16) if kind == "f16" else s).to(dev)
    rsize = {"f32": 4, "bf16": 4, "f16": 2, "f64": 8}[kind]
    o = torch.full(((elems + PAD) * rsize,), SENT, dtype=torch.uint8, device=dev)
    ob = torch.full(((elems + PAD) * 2,), SENT, dtype=torch.uint8, device=dev)
    po = o.data_ptr() if not (kind == "bf16" and outs == "bf16") else None
    pb = ob.data_ptr() if kind == "bf16" and outs != "f32" else None
    rc = B.fa_fedavg_layers_form(KIDX[kind], both.data_ptr(), both.data_ptr() + 8 * L * N, L, N, tiles, units, cap,
                                 da.data_ptr(), None if ds is None else ds.data_ptr(), float(d), po, pb,
                                 torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "fa_fedavg_layers_form", bench=True)
    ndt = {"f32": np.float32, "bf16": np.float32, "f16": F16, "f64": np.float64}[kind]

    def split(buf, dt, written):
        h = buf.cpu().numpy()
        isz = np.dtype(dt).itemsize
        keep = np.ones(h.size, bool)
        res = []
        for k in range(L):
            lo, n = int(plan[k, 1]) * isz, cols[k] * isz
            keep[lo:lo + n] = False
            res.append(h[lo:lo + n].copy().view(dt))
        assert (h[keep] == SENT).all(), "wrote outside the layers"
        assert written or (h == SENT).all()
        return res if written else [None] * L
    lf = split(o, ndt, po is not None)
    if kind != "bf16":
        return lf
    return list(zip(lf, split(ob, np.uint16, pb is not None)))


@pytest.mark.parametrize("N", [1, 9, 33])  # one row; 8 ahead plus the first; several groups and a remainder
@pytest.mark.parametrize("units", [1, 2, 4])
@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_every_form(dev, kind, scored, units, N):
    host, tens, w, sc, exp = _parity(kind, dev, N, scored)
    got = _raw(kind, dev, tens, units, 0, _factors(kind, w, sc))
    for k, (g, e) in enumerate(zip(got, exp)):
        _check_layer(kind, g, e, (kind, scored, units, N, k))


@pytest.mark.parametrize("outs", ["f32", "bf16"])
def test_bf16_single_outputs(dev, outs):
    host, tens, w, sc, exp = _parity("bf16", dev, 9, True)
    got = _raw("bf16", dev, tens, 2, 0, _factors("bf16", w, sc), outs=outs)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert (g[0] is None) == (outs == "bf16") and (g[1] is None) == (outs == "f32")
        _check_layer("bf16", g, e, (outs, k))


@pytest.mark.parametrize("units", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_grid_stride_crosses_layer_boundaries(dev, kind, units):
    """3 blocks over the 11 (units = 1) or 8 tiles of the parity model: every
    block walks through several layers."""
    host, tens, w, sc, exp = _parity(kind, dev, 9, True)
    got = _raw(kind, dev, tens, units, 3, _factors(kind, w, sc))
    for k, (g, e) in enumerate(zip(got, exp)):
        _check_layer(kind, g, e, (kind, units, k))


@pytest.mark.parametrize("kind", KINDS)
def test_unaligned_layer_between_aligned_ones(dev, kind):
    """The middle layer's rows sit one element past a 16-B boundary: it is
    folded one column per lane in the same launch, the others by units."""
    from fedlesscan_amd import engine
    u = 1 << LG[kind]
    N, seed, cols = 9, 200, [u * 256 + 5, 300, u * 256 * 2 + 3]
    host, tens = _model(kind, dev, seed, N, cols, offsets=[0, 1, 0])
    w, sc = _weights(seed, N), _scores(seed, N)
    fac = _factors(kind, w, sc)
    exp = [_literal(kind, X, *fac) for X in host]
    for e in exp:
        _meaningful(kind, e)
    for units, cap in [(1, 0), (4, 2)]:
        for k, (g, e) in enumerate(zip(_raw(kind, dev, tens, units, cap, fac), exp)):
            _check_layer(kind, g, e, (kind, units, k))
    ms = engine.ModelRowSet(_clients(tens))
    assert ms.host_plan[:, 3].tolist() == [1, 0, 1]
    got = engine.fold_model_rows(ms, w, sc)
    for k, (g, e, rows) in enumerate(zip(got, exp, tens)):
        _check_layer(kind, _engine_layer(kind, g), e, (kind, "fold_model_rows", k))
        _check_layer(kind, _engine_layer(kind, engine.fold_rows(rows, w, sc)), e, (kind, "fold_rows", k))


def _edge_layer(kind, seed, N, P):
    if kind == "bf16":
        return E.matrix_bf16(seed, N, P)
    if kind == "f64":
        return E.matrix_f64(seed, N, P)
    X = E.matrix_f32(seed, N, P)
    with np.errstate(all="ignore"):
        return X.astype(F16) if kind == "f16" else X  # float16: the float32 classes rounded to binary16


@pytest.mark.parametrize("kind", KINDS)
def test_edge_values_in_the_middle_layer(dev, kind):
    """Signed zeros, subnormals, overflow, inf, NaN and the bf16 ties
    (tests/edge_values.py, in the dtype's own format; float16: the float32
    classes rounded to binary16) as the middle layer of three, under every
    factor set."""
    u = 1 << LG[kind]
    N, seed = 9, 300
    cols = [u * 256 + 3, E.K * 21 + 4, 5]
    host, tens = _model(kind, dev, seed, N, cols)
    host[1] = _edge_layer(kind, seed, N, cols[1])
    tens[1] = [_to_dev(kind, host[1][i], dev) for i in range(N)]
    with np.errstate(all="ignore"):
        sets = list(E.factor_sets(seed, N, FDT[kind]))
    assert len(sets) == 2 * len(E.FACTOR_SETS)
    for j, (name, a, s, d) in enumerate(sets):
        got = _raw(kind, dev, tens, (1, 2, 4)[j % 3], 0, (a, s, d))
        for k, (g, X) in enumerate(zip(got, host)):
            _check_layer(kind, g, _literal(kind, X, a, s, d), (kind, E.set_id(name, s), k))
    # the edge layer did produce what it is there for
    e = _literal(kind, host[1], *sets[0][1:])
    e = np.asarray(e[0] if kind == "bf16" else e)
    assert np.isnan(e).any() and np.isinf(e).any() and (np.signbit(e) & (e == 0)).any()


# ---------------------------------------------------------------------------
# ModelRowSet / fold_model_rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_model_row_set_is_reused(dev, kind):
    """Fold, overwrite the clients' contents in place, fold again: the second
    result follows the new contents and the table is not rebuilt."""
    from fedlesscan_amd import engine
    host, tens, w, sc, exp = _parity(kind, dev, 9, True)
    tens = [[t.clone() for t in row] for row in tens]  # this test writes into them
    ms = engine.ModelRowSet(_clients(tens))
    cols = parity_cols(kind)
    assert (ms.N, ms.L, ms.sizes) == (9, len(cols), cols) and ms.dtype == _tdt(kind)
    assert not any(o % 64 for o in ms.offsets) and ms.units in (1, 2, 4)
    table, table_ptr = ms.ptrs, ms.ptrs.data_ptr()
    before = engine.stats["layer_table_folds"]
    got = engine.fold_model_rows(ms, w, sc, want_bf16=True) if kind == "bf16" else engine.fold_model_rows(ms, w, sc)
    assert engine.stats["layer_table_folds"] == before + 1
    pairs = list(zip(*got)) if kind == "bf16" else got
    assert len(pairs) == len(cols)
    for k, (g, e) in enumerate(zip(pairs, exp)):
        assert (g[0] if kind == "bf16" else g).shape == (cols[k],)
        _check_layer(kind, _engine_layer(kind, g), e, (kind, "first", k))
    # the layers are views of one flat result at the planned offsets
    flat = pairs[0][0] if kind == "bf16" else pairs[0]
    for k, g in enumerate(pairs):
        g = g[0] if kind == "bf16" else g
        if cols[k]:
            assert g.data_ptr() == flat.data_ptr() + ms.offsets[k] * flat.element_size()
    host2 = [_host_layer(kind, 777 + 10 * k, 9, P) for k, P in enumerate(cols)]
    for X, row in zip(host2, tens):
        for i, t in enumerate(row):
            t.copy_(_to_dev(kind, X[i], dev))
    got2 = engine.fold_model_rows(ms, w, sc)
    assert ms.ptrs is table and ms.ptrs.data_ptr() == table_ptr and engine.stats["layer_table_folds"] == before + 2
    fac = _factors(kind, w, sc)
    for k, (g, X) in enumerate(zip(got2, host2)):
        e = _literal(kind, X, *fac)
        _meaningful(kind, e)
        _check_layer(kind, _engine_layer(kind, g), e, (kind, "second", k))
        assert cols[k] == 0 or not _same(np.asarray(e[0] if kind == "bf16" else e),
                                         np.asarray(exp[k][0] if kind == "bf16" else exp[k]))


def test_out_over_a_client_row_and_errors(dev):
    from fedlesscan_amd import engine
    from fedlesscan_amd.aggregator.exceptions import InsufficientClientResults, InvalidParameterShapeError
    kind, N, seed, cols = "f32", 3, 400, [1030, 7]
    host, tens = _model(kind, dev, seed, N, cols)
    w = _weights(seed, N)
    exp = [_literal(kind, X, *_factors(kind, w, None)) for X in host]
    ms0 = engine.ModelRowSet(_clients(tens))
    # client 0's first layer inside the buffer the result is asked into
    big = torch.zeros(ms0.elems + cols[0], dtype=torch.float32, device=dev)
    big[ms0.elems:].copy_(tens[0][0])
    tens[0][0] = big[ms0.elems:]
    ms = engine.ModelRowSet(_clients(tens))
    assert ms.overlaps(big) and not ms.overlaps(torch.zeros(4, device=dev))
    got = engine.fold_model_rows(ms, w, out=big)
    assert got[0].data_ptr() == big.data_ptr()
    for k, (g, e) in enumerate(zip(got, exp)):
        _check_layer(kind, _engine_layer(kind, g), e, ("aliased out", k))
    assert _same(_to_host(kind, tens[0][0]), host[0][0]), "the client row was overwritten"
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_model_rows(ms, [1, 2])
    clients = _clients(tens)
    with pytest.raises(InvalidParameterShapeError):  # one client's layer of another shape
        engine.ModelRowSet([clients[0], [clients[1][0], clients[1][1][:5]], clients[2]])
    with pytest.raises(InvalidParameterShapeError):  # one dtype per model
        engine.ModelRowSet([clients[0], [t.double() for t in clients[1]], clients[2]])
    with pytest.raises(InvalidParameterShapeError):  # not contiguous
        engine.ModelRowSet([[torch.zeros(4, 6, device=dev).t()], [torch.zeros(4, 6, device=dev).t()]])
    with pytest.raises(InsufficientClientResults):
        engine.ModelRowSet([])


# ---------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------
def _surface_model(kind, dev, seed, N):
    u = 1 << LG[kind]
    shapes = [(u * 256 * 4 + 13,), (5,), (3, 7)]
    host, tens = _model(kind, dev, seed, N, [int(np.prod(s)) for s in shapes])
    params = [[t.reshape(s) for t, s in zip(cl, shapes)] for cl in _clients(tens)]
    return shapes, host, params


@pytest.mark.parametrize("strategy", ["fedavg", "stall_aware"])
@pytest.mark.parametrize("kind", KINDS)
def test_strategy_classes_take_the_layer_table(dev, kind, strategy, monkeypatch):
    from fedlesscan_amd import FedAvgAggregator, StallAwareAggregator, engine
    from fedlesscan_amd.common.models import AggregationHyperParams
    N, seed, R = 9, 500, 10
    shapes, host, params = _surface_model(kind, dev, seed, N)
    w = _weights(seed, N)
    feats = [{"round_id": r} for r in synth.round_ids(seed, N, R, 2)]
    sc = [(f["round_id"] + 1) / (R + 1) for f in feats] if strategy == "stall_aware" else None

    def run():
        if strategy == "fedavg":
            return FedAvgAggregator()._aggregate(params, w)
        return StallAwareAggregator(R, AggregationHyperParams(tolerance=2))._aggregate(feats, params, w)

    monkeypatch.setenv("FEDAVG_LAYER_TABLE", "1")
    before = dict(engine.stats)
    on = run()
    assert engine.stats["layer_table_folds"] == before["layer_table_folds"] + 1
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    assert engine.stats["rows16_folds"] - before["rows16_folds"] == (3 if kind in ("bf16", "f16") else 0)
    assert engine.stats["rows64_folds"] - before["rows64_folds"] == (3 if kind == "f64" else 0)
    monkeypatch.setenv("FEDAVG_LAYER_TABLE", "0")
    before = dict(engine.stats)
    off = run()
    assert engine.stats["layer_table_folds"] == before["layer_table_folds"]
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    fac = _factors(kind, w, sc)
    for k, (g1, g0, X) in enumerate(zip(on, off, host)):
        assert g1.is_cuda and tuple(g1.shape) == tuple(g0.shape) == shapes[k] and g1.dtype == g0.dtype == _rdt(kind)
        e = _literal(kind, X, *fac)
        _meaningful(kind, e)
        _check_layer(kind, _engine_layer(kind, g1), e, (kind, strategy, "on", k))
        _check_layer(kind, _engine_layer(kind, g0), e, (kind, strategy, "off", k))


def test_one_launch_per_dtype_group(dev, monkeypatch):
    """fp32 and bf16 layers interleaved in one model: two groups, two launches."""
    from fedlesscan_amd import engine
    N, seed = 9, 600
    _, h32, p32 = _surface_model("f32", dev, seed, N)
    _, h16, p16 = _surface_model("bf16", dev, seed + 1, N)
    params = [[a[0], b[0], a[1], b[1], a[2], b[2]] for a, b in zip(p32, p16)]
    w = _weights(seed, N)
    monkeypatch.setenv("FEDAVG_LAYER_TABLE", "1")
    before = dict(engine.stats)
    got = engine.aggregate_layers(params, w)
    assert engine.stats["layer_table_folds"] == before["layer_table_folds"] + 2
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    for k in range(3):
        _check_layer("f32", _engine_layer("f32", got[2 * k]), _literal("f32", h32[k], *_factors("f32", w, None)), k)
        _check_layer("bf16", _engine_layer("bf16", got[2 * k + 1]),
                     _literal("bf16", h16[k], *_factors("bf16", w, None)), k)


# ---------------------------------------------------------------------------
# fallbacks
# ---------------------------------------------------------------------------
def test_float16_numpy_scalar_weights_still_promote(dev, monkeypatch):
    """float16 layers under np.float32 weights: numpy promotes the fold to
    float32, no table fold does that; the layers come back float32 with
    numpy's bits, from aggregate_layers and from fold_model_rows."""
    from fedlesscan_amd import engine
    N, seed = 9, 700
    shapes, host, params = _surface_model("f16", dev, seed, N)
    w32 = [np.float32(v) for v in _weights(seed, N)]
    exp = O.fedavg_literal([[X[i].reshape(s) for X, s in zip(host, shapes)] for i in range(N)], w32)
    monkeypatch.setenv("FEDAVG_LAYER_TABLE", "1")
    before = dict(engine.stats)
    for got in (engine.aggregate_layers(params, w32), engine.fold_model_rows(params, w32)):
        assert engine.stats["layer_table_folds"] == before["layer_table_folds"]
        assert engine.stats["rows16_folds"] == before["rows16_folds"]
        for g, e in zip(got, exp):
            assert e.dtype == np.float32 and g.dtype == torch.float32 and tuple(g.shape) == e.shape
            assert _same(g.cpu().numpy(), e)


@pytest.mark.parametrize("kind", ["bf16", "f64"])
def test_one_layer_group_keeps_the_row_table(dev, kind, monkeypatch):
    from fedlesscan_amd import engine
    N, seed = 9, 800
    host, tens = _model(kind, dev, seed, N, [1000])
    w = _weights(seed, N)
    monkeypatch.setenv("FEDAVG_LAYER_TABLE", "1")
    before = dict(engine.stats)
    got = engine.aggregate_layers(_clients(tens), w)
    assert engine.stats["layer_table_folds"] == before["layer_table_folds"]
    key = "rows16_folds" if kind == "bf16" else "rows64_folds"
    assert engine.stats[key] == before[key] + 1
    _check_layer(kind, _engine_layer(kind, got[0]), _literal(kind, host[0], *_factors(kind, w, None)), kind)


def test_capture_takes_the_per_layer_route(dev):
    """Under torch.cuda.graph fold_model_rows folds bf16 layers one fold_rows
    each, over the set's own table (nothing is uploaded inside the capture),
    and the replays stay exact; float16 keeps fold_rows' refusal."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    N, seed, cols = 9, 850, [8 * 256 + 5, 40, 1]

    def model(kind, scored):
        host, tens = _model(kind, dev, seed, N, cols)
        w, sc = _weights(seed, N), (_scores(seed, N) if scored else None)
        return tens, w, sc, [_literal(kind, X, *_factors(kind, w, sc)) for X in host]

    tens, w, sc, exp = model("bf16", True)
    ms = engine.ModelRowSet(_clients(tens))
    for k, g in enumerate(engine.fold_model_rows(ms, w, sc)):
        _meaningful("bf16", exp[k])
        _check_layer("bf16", _engine_layer("bf16", g), exp[k], ("eager", k))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    before = dict(engine.stats)
    with torch.cuda.graph(g, stream=side):
        outs = engine.fold_model_rows(ms, w, sc)
    assert engine.stats["layer_table_folds"] == before["layer_table_folds"]
    assert engine.stats["rows16_folds"] == before["rows16_folds"] + sum(1 for n in ms.sizes if n)
    for _ in range(3):
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            _check_layer("bf16", _engine_layer("bf16", o), exp[k], ("replay", k))
    tens, w, sc, exp = model("f16", False)
    ms = engine.ModelRowSet(_clients(tens))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(InvalidParameterShapeError, match="capture"):
        with torch.cuda.graph(g, stream=side):
            engine.fold_model_rows(ms, w)
    torch.cuda.synchronize()
    for k, o in enumerate(engine.fold_model_rows(ms, w)):
        _check_layer("f16", _engine_layer("f16", o), exp[k], ("after the refused capture", k))


# ---------------------------------------------------------------------------
# memory: no stacked copy
# ---------------------------------------------------------------------------
def test_no_stacking_copy_in_memory(dev):
    """32 clients x three bf16 layers of 256K (48 MB): one fold_model_rows
    raises the peak of allocated memory by less than half the input's bytes."""
    from fedlesscan_amd import engine
    N, P, L = 32, 1 << 18, 3
    gen = torch.Generator(device=dev).manual_seed(9)
    params = [[(torch.randn(P, device=dev, generator=gen) * 0.05).to(torch.bfloat16) for _ in range(L)]
              for _ in range(N)]
    w = _weights(900, N)
    ms = engine.ModelRowSet(params)
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    outs = engine.fold_model_rows(ms, w)
    torch.cuda.synchronize(dev)
    rise = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak rise {rise} bytes for {2 * N * P * L} input bytes")
    assert rise < N * P * L, rise
    for k, o in enumerate(outs):
        ref = engine.fold_rows([params[i][k] for i in range(N)], w)
        assert o.dtype == torch.float32 and torch.equal(o.view(torch.int32), ref.view(torch.int32))
        assert torch.isfinite(o).all() and (o.abs() >= 2.0 ** -14).any()
