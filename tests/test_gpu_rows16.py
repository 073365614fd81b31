"""GPU parity of the 16-bit row-table folds (fa_fedavg_bf16_ptrs,
fa_fedavg_f16_ptrs) and of the routes that reach them: engine.fold_rows,
aggregate_layers and the strategy classes.  Every comparison is bit for bit.

Expected values
  bf16     oracle.fedavg_stacked_bf16 on the rows' bit patterns (the float32
           result and its RNE bf16 copy); inputs finite.
  float16  numpy's own binary16 fold (oracle.fedavg_stacked on float16 rows with
           Python-number factors: layer * n [* s], left-to-right np.add,
           / total); NaN positions as a mask, every other bit pattern exactly.
Each expectation is also what fold_stacked gives over the same rows stacked
(checked once per shape, where the expectation is made).  Inputs come from
fedlesscan_amd.synth."""
import functools

import numpy as np
import pytest

from fedlesscan_amd import synth
from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F16 = np.float16
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A  # an element no kernel writes keeps this pattern
PAD = 8  # sentinel elements behind every output
# one row; no full group; group + remainder for 2, 8 and 16 rows ahead; the first row apart;
# 4 and 10: the first row, exactly one group of 2 / 8 rows ahead, one leftover row
NS = [1, 2, 4, 9, 10, 17, 18, 33]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# inputs and expectations, made once per shape and shared
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bits(kind: str, seed: int, N: int, P: int) -> np.ndarray:
    """[N, P] uint16 bit patterns of the rows: bf16 (RNE of the generator) or binary16."""
    X = synth.clients_f32(seed, N, 0, P)
    b = synth.f32_to_bf16_bits(X) if kind == "bf16" else X.astype(F16).view(np.uint16)
    b.setflags(write=False)
    return b


def _weights(seed, N):
    return synth.cardinalities(seed, N)  # 1..600: 33 of them sum below 65504, the binary16 divisor stays finite


def _scores(seed, N, R=10):
    return [(r + 1) / (R + 1) for r in synth.round_ids(seed, N, R, 2)]


def _oracle(kind, bits, w, sc=None, total=None):
    """(float32 result, RNE bf16 bits) for bf16 rows, the binary16 result for float16 rows."""
    if kind == "bf16":
        return O.fedavg_stacked_bf16(bits, w, sc, total)
    with np.errstate(all="ignore"):
        e = O.fedavg_stacked(bits.view(F16), w, sc, total)
    assert e.dtype == F16
    return e


def same_bits32(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32),
                                                                                      b.view(np.uint32))


def same_bits16(a, b) -> bool:
    """float16: equal NaN positions, equal bit patterns everywhere else (as tests/test_gpu_f16.py)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F16 or b.dtype != F16 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~na]))


def _meaningful(kind, exp) -> None:
    """Parity is never satisfied by zeros, infinities or NaNs alone."""
    e = np.asarray(exp[0] if kind == "bf16" else exp, dtype=np.float32)
    assert np.isfinite(e).all() and (np.abs(e) >= 2.0 ** -14).any()


def _torch_dt(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float16


def _dev16(bits: np.ndarray, kind, dev):
    """uint16 bit patterns as a CUDA tensor of the kind's dtype."""
    return torch.from_numpy(np.array(bits, dtype=np.uint16).view(np.int16)).to(dev).view(_torch_dt(kind))


def _host16(t) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _check(kind, got, exp, what) -> None:
    """got: the kind's result(s) as fold_rows / fold_stacked return them (CUDA tensors)."""
    if kind == "f16":
        assert got.dtype == torch.float16
        assert same_bits16(_host16(got).view(F16), exp), what
        return
    ef, eb = exp
    if isinstance(got, tuple):
        f, b = got
    else:
        f, b = (got, None) if got.dtype == torch.float32 else (None, got)
    assert f is not None or b is not None
    if f is not None:
        assert f.dtype == torch.float32 and same_bits32(f.cpu().numpy(), ef), what
    if b is not None:
        assert b.dtype == torch.bfloat16 and np.array_equal(_host16(b), eb), what


_EXPECT: dict = {}


def _expect(kind, dev, seed, N, P, scored):
    """The expectation for rows _bits(kind, seed, N, P) under _weights / _scores
    (seed), made once per shape; it is also what fold_stacked gives over the
    same rows stacked."""
    key = (kind, seed, N, P, scored)
    if key not in _EXPECT:
        from fedlesscan_amd import engine
        bits = _bits(kind, seed, N, P)
        w, sc = _weights(seed, N), (_scores(seed, N) if scored else None)
        exp = _oracle(kind, bits, w, sc)
        _meaningful(kind, exp)
        X = _dev16(bits, kind, dev)
        _check(kind, engine.fold_stacked(X, w, sc, want_bf16=True) if kind == "bf16" else
               engine.fold_stacked(X, w, sc), exp, ("fold_stacked", key))
        _EXPECT[key] = exp
    return _EXPECT[key]


def _separate_rows(kind, dev, bits):
    """Each row its own allocation (16-B aligned, as the allocator gives them)."""
    rows = [_dev16(bits[i].copy(), kind, dev) for i in range(bits.shape[0])]
    assert all(r.data_ptr() % 16 == 0 for r in rows)
    return rows


def _table(rows, dev):
    return torch.tensor([r.data_ptr() for r in rows], dtype=torch.int64, device=dev)


def _factors_dev(kind, dev, w, sc):
    """Device factor arrays and the divisor argument of the raw entries."""
    if kind == "bf16":
        a = torch.tensor(np.array(w, np.float32), device=dev)
        s = None if sc is None else torch.tensor(np.array(sc, np.float32), device=dev)
        return a, s, float(np.float32(sum(w)))
    with np.errstate(all="ignore"):
        a = _dev16(np.array([F16(v) for v in w], F16).view(np.uint16), "f16", dev)
        s = None if sc is None else _dev16(np.array([F16(v) for v in sc], F16).view(np.uint16), "f16", dev)
        return a, s, int(np.asarray(F16(sum(w))).view(np.uint16))


def _raw(kind, dev, tab, N, P, fac, aligned, form, outs="both", off=0):
    """The bench-library entry (form by index, -1 the policy) over the table;
    returns the outputs on the host after checking the sentinels around them.
    outs (bf16): "f32", "bf16" or "both"; off: element offset of the outputs."""
    from fedlesscan_amd import _lib
    B = _lib.load_bench()
    a, s, d = fac
    st = torch.cuda.current_stream(dev).cuda_stream
    sp = None if s is None else s.data_ptr()
    o16 = torch.full((P + PAD + off,), SENT16, dtype=torch.int16, device=dev)
    if kind == "f16":
        rc = B.fa_fedavg_f16_ptrs_form(tab.data_ptr(), N, P, a.data_ptr(), sp, d, aligned, o16.data_ptr() + 2 * off,
                                       st, form)
        _lib.check(rc, "fa_fedavg_f16_ptrs_form", bench=True)
        h = o16.cpu().numpy().view(np.uint16)
        assert (h[:off] == SENT16).all() and (h[off + P:] == SENT16).all(), "wrote outside out"
        return h[off:off + P].view(F16)
    o32 = torch.full((P + PAD + off,), SENT32, dtype=torch.int32, device=dev)
    rc = B.fa_fedavg_bf16_ptrs_form(tab.data_ptr(), N, P, a.data_ptr(), sp, d, aligned,
                                    o32.data_ptr() + 4 * off if outs != "bf16" else None,
                                    o16.data_ptr() + 2 * off if outs != "f32" else None, st, form)
    _lib.check(rc, "fa_fedavg_bf16_ptrs_form", bench=True)
    h32, h16 = o32.cpu().numpy().view(np.uint32), o16.cpu().numpy().view(np.uint16)
    assert (h32[:off] == SENT32).all() and (h32[off + P:] == SENT32).all(), "wrote outside out_f32"
    assert (h16[:off] == SENT16).all() and (h16[off + P:] == SENT16).all(), "wrote outside out_bf16"
    assert outs != "bf16" or (h32 == SENT32).all()
    assert outs != "f32" or (h16 == SENT16).all()
    return (h32[off:off + P].view(np.float32) if outs != "bf16" else None,
            h16[off:off + P] if outs != "f32" else None)


def _check_raw(kind, got, exp, what) -> None:
    if kind == "f16":
        assert same_bits16(got, exp), what
        return
    f, b = got
    if f is not None:
        assert same_bits32(f, exp[0]), what
    if b is not None:
        assert np.array_equal(b, exp[1]), what


def _forms():
    """[(index, name, columns per tile)]: 8 * 256 * C for the octet forms, 256 for the column form."""
    from fedlesscan_amd import _lib
    B = _lib.load_bench()
    out = []
    for f in range(B.fa_num_rows16_forms()):
        name = B.fa_rows16_form_name(f).decode()
        out.append((f, name, 256 if name.endswith("column") else 8 * 256 * int(name.rsplit("c", 1)[1])))
    assert len(out) >= 5 and sorted(t for _, _, t in out) == [256, 2048, 4096, 8192, 16384]
    return out


def _edge_sizes(T):
    # T + 11: a full tile, a last tile with exactly one octet, a 3-column tail
    return [1, 7, 8, 9, T - 1, T, T + 11, T + 13]


# ---------------------------------------------------------------------------
# 1. every form by index, and the policy, at the tile edges of each form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_every_form_at_its_tile_edges(dev, kind, N):
    """Each (rows ahead, octets per lane) form and the column form through the
    bench-library entry, at P = 1, 7, 8, 9, T - 1, T, T + 11, T + 13 for the form's
    tile of T columns, FedAvg and scored; bf16 with out_f32 only, out_bf16 only
    and both.  The policy (-1) runs the same sizes with the rows promised
    aligned and not.  The rows are uploaded once at the largest P; a smaller P
    folds their first P elements."""
    forms = _forms()
    Pmax = max(T for _, _, T in forms) + 13
    seed = 100 + N
    rows = _separate_rows(kind, dev, _bits(kind, seed, N, Pmax))
    tab = _table(rows, dev)
    w = _weights(seed, N)
    runs = [(f, name, _edge_sizes(T), (0, 1) if T == 256 else (1,)) for f, name, T in forms]
    runs.append((-1, "policy", sorted(set(_edge_sizes(2048) + _edge_sizes(16384))), (0, 1)))
    for scored in (False, True):
        sc = _scores(seed, N) if scored else None
        fac = _factors_dev(kind, dev, w, sc)
        for f, name, sizes, promises in runs:
            for P in sizes:
                key = (kind, seed, N, P, scored)
                if key not in _EXPECT:  # the rows' first P columns: columns are independent
                    _EXPECT[key] = _expect_prefix(kind, dev, _bits(kind, seed, N, Pmax)[:, :P], w, sc)
                for aligned in promises:
                    for outs in (("f32", "bf16", "both") if kind == "bf16" else ("both",)):
                        got = _raw(kind, dev, tab, N, P, fac, aligned, f, outs)
                        _check_raw(kind, got, _EXPECT[key], (name, N, P, scored, aligned, outs))


def _expect_prefix(kind, dev, bits, w, sc):
    from fedlesscan_amd import engine
    exp = _oracle(kind, np.ascontiguousarray(bits), w, sc)
    _meaningful(kind, exp)
    X = _dev16(bits, kind, dev)
    _check(kind, engine.fold_stacked(X, w, sc, want_bf16=True) if kind == "bf16" else engine.fold_stacked(X, w, sc),
           exp, ("fold_stacked", bits.shape))
    return exp


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_more_tiles_than_blocks(dev, kind):
    """P = 2048 * (CUs + 3) + 5 with 3 rows: more one-octet tiles than the grid
    has blocks, so the narrowest octet form (and the policy, which picks it
    here) walks the grid-stride loop; the 5 trailing columns fall to one lane."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    N, P, seed = 3, 2048 * (cus + 3) + 5, 7
    c1 = [f for f, name, T in _forms() if T == 2048]
    assert len(c1) == 1
    rows = _separate_rows(kind, dev, _bits(kind, seed, N, P))
    tab = _table(rows, dev)
    for scored in (False, True):
        exp = _expect(kind, dev, seed, N, P, scored)
        fac = _factors_dev(kind, dev, _weights(seed, N), _scores(seed, N) if scored else None)
        for f in (c1[0], -1):
            _check_raw(kind, _raw(kind, dev, tab, N, P, fac, 1, f), exp, (f, scored))


# ---------------------------------------------------------------------------
# 2. where the rows lie: engine.fold_rows / RowSet
# ---------------------------------------------------------------------------
P_ROWS = 8 * 256 + 13  # a full one-octet tile, one more octet, 5 trailing columns


@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("place", ["separate", "permuted", "twice", "odd_row", "out_offset", "pitch16", "pitch_odd"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_row_placement(dev, kind, place, scored):
    """separate: each row its own allocation.  permuted: rows cut from one
    buffer and listed in another order (the table's order decides, not the
    addresses).  twice: one tensor listed twice.  odd_row: one row at an odd
    element offset among aligned ones, so the whole call takes the column form.
    out_offset: out 2 bytes off 16-B alignment, likewise.  pitch16 / pitch_odd:
    rows of one buffer at a constant pitch that is / is not a multiple of 16
    bytes: the strided view and the stacked fold, no table."""
    from fedlesscan_amd import engine
    N, P, seed = 9, P_ROWS, 31
    bits = _bits(kind, seed, N, P)
    w, sc = _weights(seed, N), (_scores(seed, N) if scored else None)
    order = list(range(N))
    out = None
    table, aligned = True, True
    if place == "separate":
        rows = _separate_rows(kind, dev, bits)
    elif place == "permuted":
        pitch = (P + 7) // 8 * 8
        buf = torch.zeros(N * pitch, dtype=_torch_dt(kind), device=dev)
        buf.view(N, pitch)[:, :P].copy_(_dev16(bits, kind, dev))
        order = [int(i) for i in np.random.default_rng(5).permutation(N)]
        assert order != sorted(order)
        rows = [buf[i * pitch:i * pitch + P] for i in order]
    elif place == "twice":
        rows = _separate_rows(kind, dev, bits)
        order = [0, 1, 0, 2, 3, 3, 4, 5, 0]
        rows = [rows[i] for i in order]
    elif place == "odd_row":
        rows = _separate_rows(kind, dev, bits)
        holder = torch.zeros(P + 1, dtype=_torch_dt(kind), device=dev)
        holder[1:].copy_(rows[4])
        rows[4] = holder[1:]
        assert rows[4].data_ptr() % 16 == 2
        aligned = False
    elif place == "out_offset":
        rows = _separate_rows(kind, dev, bits)
        # the 16-bit output one element off (a float32 tensor cannot sit 2 bytes off)
        out_base = torch.zeros(P + 8, dtype=_torch_dt(kind), device=dev)
        out = out_base[1:P + 1]
        assert out.data_ptr() % 16 == 2
    else:
        pitch = (P + 7) // 8 * 8 if place == "pitch16" else P + 1
        assert (pitch * 2) % 16 == (0 if place == "pitch16" else 12)
        buf = torch.zeros(N * pitch, dtype=_torch_dt(kind), device=dev)
        buf.view(N, pitch)[:, :P].copy_(_dev16(bits, kind, dev))
        rows = [buf[i * pitch:i * pitch + P] for i in range(N)]
        table = False
    rs = engine.RowSet(rows)
    assert (rs.view is None) == table
    if table:
        assert rs.ptrs is not None and rs.aligned == aligned
    wo, sco = [w[i] for i in order], (None if sc is None else [sc[i] for i in order])
    exp = _oracle(kind, np.ascontiguousarray(bits[order]), wo, sco, sum(wo))
    _meaningful(kind, exp)
    before = dict(engine.stats)
    if kind == "bf16":
        got = engine.fold_rows(rs, wo, sco, want_bf16=True) if out is None else engine.fold_rows(rs, wo, sco,
                                                                                                 out_bf16=out)
    else:
        got = engine.fold_rows(rs, wo, sco, out=out)
    if out is not None:
        assert got is out
        assert _host16(out_base)[0] == 0 and (_host16(out_base)[P + 1:] == 0).all()  # nothing written outside out
    _check(kind, got, exp, (kind, place, scored))
    assert engine.stats["rows16_folds"] - before["rows16_folds"] == (1 if table else 0)
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    # the same rows stacked give the same bits
    X = torch.stack(list(rows))
    _check(kind, engine.fold_stacked(X, wo, sco, want_bf16=True) if kind == "bf16" else engine.fold_stacked(X, wo, sco),
           exp, ("stacked", kind, place, scored))


@pytest.mark.parametrize("kind", ["bf16", "f16", "bf16_f32out"])
def test_out_over_a_row(dev, kind):
    """An output that overlaps a client row: the table lives in device memory,
    so fold_rows folds into a fresh buffer and copies.  The result equals the
    call with its own output, and the other rows keep their contents.
    bf16_f32out: the float32 output shares its first bytes with a bf16 row."""
    from fedlesscan_amd import engine
    k = "bf16" if kind.startswith("bf16") else "f16"
    N, P, seed, hit = 9, P_ROWS, 33, 4
    bits = _bits(k, seed, N, P)
    w, sc = _weights(seed, N), _scores(seed, N)
    rows = _separate_rows(k, dev, bits)
    if kind == "bf16_f32out":
        store = torch.zeros(P, dtype=torch.float32, device=dev)
        rows[hit] = store.view(torch.bfloat16)[:P]
        rows[hit].copy_(_dev16(bits[hit].copy(), k, dev))
    rs = engine.RowSet(rows)
    assert rs.view is None and rs.aligned
    exp = _oracle(k, bits, w, sc)
    _meaningful(k, exp)
    clean = engine.fold_rows(rs, w, sc, want_bf16=True) if k == "bf16" else engine.fold_rows(rs, w, sc)
    _check(k, clean, exp, "own output")
    if kind == "bf16":
        assert rs.overlaps(rows[hit])
        got = engine.fold_rows(rs, w, sc, out_bf16=rows[hit])
        assert got is rows[hit]
    elif kind == "bf16_f32out":
        assert rs.overlaps(store)
        got = engine.fold_rows(rs, w, sc, out=store)
        assert got is store
    else:
        got = engine.fold_rows(rs, w, sc, out=rows[hit])
        assert got is rows[hit]
    _check(k, got, exp, "output over a row")
    for i in range(N):
        if i != hit:
            assert np.array_equal(_host16(rows[i]), bits[i]), i


# ---------------------------------------------------------------------------
# 3. the public surface
# ---------------------------------------------------------------------------
LAYERS = [8 * 256 * 4 + 13, 5]


def _client_layers(kind, seed, N):
    """N clients x two layers, as bit patterns."""
    return [[_bits(kind, seed + 10 * li, N, n)[i] for li, n in enumerate(LAYERS)] for i in range(N)]


@pytest.mark.parametrize("strategy", ["fedavg", "stall_aware"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_strategy_classes_fold_through_the_row_tables(dev, kind, strategy):
    from fedlesscan_amd import FedAvgAggregator, StallAwareAggregator, engine
    from fedlesscan_amd.common.models import AggregationHyperParams
    N, seed, R = 9, 41, 10
    layers = _client_layers(kind, seed, N)
    params = [[_dev16(x.copy(), kind, dev) for x in cl] for cl in layers]
    w = _weights(seed, N)
    feats = [{"round_id": r} for r in synth.round_ids(seed, N, R, 2)]
    sc = [(f["round_id"] + 1) / (R + 1) for f in feats] if strategy == "stall_aware" else None
    before = dict(engine.stats)
    if strategy == "fedavg":
        got = FedAvgAggregator()._aggregate(params, w)
    else:
        got = StallAwareAggregator(R, AggregationHyperParams(tolerance=2))._aggregate(feats, params, w)
    assert engine.stats["rows16_folds"] - before["rows16_folds"] == len(LAYERS)
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    assert len(got) == len(LAYERS)
    for li, g in enumerate(got):
        exp = _oracle(kind, np.stack([cl[li] for cl in layers]), w, sc)
        _meaningful(kind, exp)
        assert g.is_cuda and tuple(g.shape) == (LAYERS[li],)
        assert g.dtype == (torch.float32 if kind == "bf16" else torch.float16)
        _check(kind, g, exp, (kind, strategy, li))


def test_float16_numpy_scalar_weights_still_promote(dev):
    """float16 layers under np.float32 weights: numpy promotes the fold to
    float32, no row-table fold does that, so the group is stacked as before."""
    from fedlesscan_amd import FedAvgAggregator, engine
    N, seed = 9, 43
    layers = _client_layers("f16", seed, N)
    params = [[_dev16(x.copy(), "f16", dev) for x in cl] for cl in layers]
    w32 = [np.float32(v) for v in _weights(seed, N)]
    exp = O.fedavg_literal([[x.view(F16) for x in cl] for cl in layers], w32)
    before = dict(engine.stats)
    got = FedAvgAggregator()._aggregate(params, w32)
    assert engine.stats["rows16_folds"] == before["rows16_folds"]
    assert engine.stats["stacked_groups"] == before["stacked_groups"] + 1
    for g, e in zip(got, exp):
        assert e.dtype == np.float32 and g.dtype == torch.float32 and same_bits32(g.cpu().numpy(), e)
    # fold_rows itself: the stacked fallback
    rows = [p[0] for p in params]
    g = engine.fold_rows(rows, w32)
    assert engine.stats["rows16_folds"] == before["rows16_folds"]
    assert g.dtype == torch.float32 and same_bits32(g.cpu().numpy(), exp[0])


# ---------------------------------------------------------------------------
# 4. memory: no stacked copy
# ---------------------------------------------------------------------------
def test_no_stacking_copy_in_memory(dev):
    """64 rows of 1M bf16 (128 MB): one fold_rows raises the peak of allocated
    memory by less than N * P bytes, half the input's size -- a stacked copy
    alone needs 2 * N * P bytes.  Rows are generated on the device (the
    library's own generator, bit-identical to synth); the result equals the
    stacked fold over the same rows."""
    from fedlesscan_amd import _lib, engine
    B = _lib.load_bench()
    N, P, seed = 64, 1 << 20, 51
    st = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for i in range(N):
        r = torch.empty(P, dtype=torch.bfloat16, device=dev)
        _lib.check(B.fa_synth_bf16(r.data_ptr(), 1, P, P, seed, i, 0, st), "fa_synth_bf16", bench=True)
        rows.append(r)
    assert np.array_equal(_host16(rows[3][:4096]), synth.clients_bf16(seed, 1, 0, 4096, row0=3)[0])
    w = _weights(seed, N)
    rs = engine.RowSet(rows)
    assert rs.view is None and rs.aligned
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = engine.fold_rows(rs, w)
    torch.cuda.synchronize(dev)
    rise = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak rise {rise} bytes for {2 * N * P} input bytes")
    assert rise < N * P, rise
    ref = engine.fold_stacked(torch.stack(rows), w)
    assert out.dtype == torch.float32 and torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert torch.isfinite(out).all() and (out.abs() >= 2.0 ** -14).any()


# ---------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------
def test_bf16_row_fold_captures_and_replays(dev):
    from fedlesscan_amd import engine
    N, P, seed = 33, P_ROWS, 61
    bits = _bits("bf16", seed, N, P)
    w, sc = _weights(seed, N), _scores(seed, N)
    exp = _expect("bf16", dev, seed, N, P, True)
    rs = engine.RowSet(_separate_rows("bf16", dev, bits))
    _check("bf16", engine.fold_rows(rs, w, sc, want_bf16=True), exp, "eager")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    before = engine.stats["rows16_folds"]
    with torch.cuda.graph(g, stream=side):
        out, outb = engine.fold_rows(rs, w, sc, want_bf16=True)
    assert engine.stats["rows16_folds"] == before + 1
    for _ in range(3):
        out.fill_(float("nan"))
        outb.zero_()
        g.replay()
        torch.cuda.synchronize()
        _check("bf16", (out, outb), exp, "replay")


def test_float16_row_fold_refuses_capture(dev):
    from fedlesscan_amd import engine
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    N, P, seed = 9, 40, 63
    bits = _bits("f16", seed, N, P)
    w = _weights(seed, N)
    rs = engine.RowSet(_separate_rows("f16", dev, bits))
    assert rs.view is None
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(InvalidParameterShapeError, match="capture"):
        with torch.cuda.graph(g, stream=side):
            engine.fold_rows(rs, w)
    torch.cuda.synchronize()
    _check("f16", engine.fold_rows(rs, w), _oracle("f16", bits, w), "after the refused capture")


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_errors(dev):
    from fedlesscan_amd import _lib, engine
    from fedlesscan_amd.aggregator.exceptions import InsufficientClientResults, InvalidParameterShapeError
    L = _lib.load()
    N, P, seed = 3, 40, 65
    st = torch.cuda.current_stream(dev).cuda_stream
    for kind in ("bf16", "f16"):
        rows = _separate_rows(kind, dev, _bits(kind, seed, N, P))
        tab = _table(rows, dev)
        a, _, d = _factors_dev(kind, dev, _weights(seed, N), None)
        if kind == "bf16":
            assert L.fa_fedavg_bf16_ptrs(tab.data_ptr(), N, P, a.data_ptr(), None, d, 1, None, None, st) == \
                _lib.FA_ERR_ARG
            assert L.fa_fedavg_bf16_ptrs(tab.data_ptr(), 0, P, a.data_ptr(), None, d, 1, a.data_ptr(), None, st) == \
                _lib.FA_ERR_NO_CLIENTS
            host = np.array(_weights(seed, N), np.float32)
            assert L.fa_fedavg_bf16_ptrs_hostf(tab.data_ptr(), N, P, host.ctypes.data, None, d, 1, None, None,
                                               st) == _lib.FA_ERR_ARG
        else:
            assert L.fa_fedavg_f16_ptrs(tab.data_ptr(), 0, P, a.data_ptr(), None, d, 1, a.data_ptr(), st) == \
                _lib.FA_ERR_NO_CLIENTS
            assert L.fa_fedavg_f16_ptrs(tab.data_ptr(), N, P, a.data_ptr(), None, d, 1, None, st) == _lib.FA_ERR_ARG
        with pytest.raises(InsufficientClientResults):
            _lib.check(_lib.FA_ERR_NO_CLIENTS, "status mapping")
        with pytest.raises(InvalidParameterShapeError):
            engine.fold_rows(rows, [1, 2])
        with pytest.raises(InvalidParameterShapeError):
            engine.fold_rows(rows, [1, 2, 3], [0.5, 1.0])
        wrong = torch.empty(P, dtype=torch.float64, device=dev)
        with pytest.raises(ValueError):
            engine.fold_rows(rows, [1, 2, 3], out=wrong)
        good = torch.float32 if kind == "bf16" else torch.float16
        with pytest.raises(ValueError):
            engine.fold_rows(rows, [1, 2, 3], out=torch.empty(P - 1, dtype=good, device=dev))
        with pytest.raises(ValueError):
            engine.fold_rows(rows, [1, 2, 3], out=torch.empty(2 * P, dtype=good, device=dev)[::2])
        if kind == "bf16":
            with pytest.raises(ValueError):
                engine.fold_rows(rows, [1, 2, 3], out_bf16=torch.empty(P, dtype=torch.float16, device=dev))
        else:
            with pytest.raises(InvalidParameterShapeError):
                engine.fold_rows(rows, [1, 2, 3], out_bf16=torch.empty(P, dtype=torch.bfloat16, device=dev))
    torch.cuda.synchronize()
