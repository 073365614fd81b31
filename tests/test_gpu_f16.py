"""GPU parity of the float16 fold (fa_fedavg_f16) against numpy itself.

numpy keeps a float16 layer float16 under Python-number weights (NEP 50), so
the reference multiplies, adds and divides in binary16; oracle.fedavg_oracle is
dtype-generic and is the checker.  Contract: equal NaN positions (sign and
payload free: x86 numpy makes the negative default NaN, the GPU the positive
one) and equal bit patterns everywhere else, which covers signed zeros,
subnormals and infinities."""
import numpy as np
import pytest

from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F16 = np.float16
SENTINEL = 0x5A5A  # an element the kernel never writes keeps this pattern


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def same_bits16(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F16 or b.dtype != F16 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~na]))


def _describe(got, exp):
    na, nb = np.isnan(got), np.isnan(exp)
    bad = np.flatnonzero((na != nb) | ((got.view(np.uint16) != exp.view(np.uint16)) & ~(na & nb)))
    i = int(bad[0]) if bad.size else -1
    return f"{bad.size} differ; first col {i}: got {got.view(np.uint16)[i]:#06x} exp {exp.view(np.uint16)[i]:#06x}"


def _half(v) -> np.float16:
    with np.errstate(all="ignore"):
        return F16(v)


def _dev_bits(x: np.ndarray, dev):
    """A float16 numpy array as a CUDA float16 tensor (through its bit pattern)."""
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).to(dev).view(torch.float16)


def _host(t) -> np.ndarray:
    return t.view(torch.int16).cpu().numpy().view(F16)


def _raw(dev, Xd, P, a, s, d, form=None):
    """fa_fedavg_f16 (form None) or fa_fedavg_f16_form over the rows of Xd
    ([N, ldx] CUDA float16) with binary16 factors a, s (numpy) and divisor d."""
    from fedlesscan_amd import _lib
    N, ldx = Xd.shape
    ad = _dev_bits(np.asarray(a, F16), dev)
    sd = None if s is None else _dev_bits(np.asarray(s, F16), dev)
    out = torch.full((P,), SENTINEL, dtype=torch.int16, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    dbits = int(np.asarray(d, F16).view(np.uint16))
    sp = None if sd is None else sd.data_ptr()
    if form is None:
        _lib.check(_lib.load().fa_fedavg_f16(Xd.data_ptr(), N, P, ldx, ad.data_ptr(), sp, dbits, out.data_ptr(), st),
                   "fa_fedavg_f16")
    else:
        _lib.check(_lib.load_bench().fa_fedavg_f16_form(Xd.data_ptr(), N, P, ldx, ad.data_ptr(), sp, dbits,
                                                        out.data_ptr(), st, form), "fa_fedavg_f16_form", bench=True)
    return out.cpu().numpy().view(F16)


def _oracle(X, w, s=None, total=None):
    with np.errstate(all="ignore"):
        return O.fedavg_stacked(X, w, s, total)


# ---------------------------------------------------------------------------
# 1. every binary16 operand of each operation, one column per bit pattern
# ---------------------------------------------------------------------------
ALL = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(F16)


@pytest.fixture(scope="module")
def all_patterns(dev):
    return _dev_bits(ALL.reshape(1, -1), dev)


@pytest.mark.parametrize("a", [1, 3, 0.1, 6.1e-5, 65504, float("inf")])
def test_exhaustive_multiply(dev, all_patterns, a):
    """out = fl16(x * a) [then * s] for every x (N = 1, d = 1): 6.1e-5 puts the
    products of normal operands into the subnormal range, 65504 and inf
    overflow."""
    ah = _half(a)
    got = _raw(dev, all_patterns, 65536, [ah], None, F16(1))
    exp = _oracle(ALL.reshape(1, -1), [float(ah)], None, 1.0)
    assert exp.dtype == F16 and same_bits16(got, exp), (a, _describe(got, exp))
    for s in (0.5, 1 / 3):
        sh = _half(s)
        got = _raw(dev, all_patterns, 65536, [ah], [sh], F16(1))
        exp = _oracle(ALL.reshape(1, -1), [float(ah)], [float(sh)], 1.0)
        assert same_bits16(got, exp), (a, s, _describe(got, exp))


@pytest.mark.parametrize("d", [1, 3, 7, 1000, 65504, 6e-8, float("inf")])
def test_exhaustive_divide(dev, all_patterns, d):
    """out = fl16(x / d) for every x (N = 1, a = 1): certifies the divide
    sequence the kernels ship (float32 IEEE divide, one rounding to half)."""
    dh = _half(d)
    got = _raw(dev, all_patterns, 65536, [F16(1)], None, dh)
    exp = _oracle(ALL.reshape(1, -1), [1.0], None, float(dh))
    assert exp.dtype == F16 and same_bits16(got, exp), (d, _describe(got, exp))


@pytest.mark.parametrize("c", [1, -1, 2.0 ** -14, 6e-8, 1024.5, 65504, -65504])
def test_exhaustive_add(dev, c):
    """out = fl16(x + c) for every x (N = 2, a = (1, 1), d = 1): cancellation
    to +-0, the subnormal boundary, overflow to inf."""
    X = np.stack([ALL, np.full(65536, _half(c), F16)])
    got = _raw(dev, _dev_bits(X, dev), 65536, [F16(1), F16(1)], None, F16(1))
    exp = _oracle(X, [1.0, 1.0], None, 1.0)
    assert exp.dtype == F16 and same_bits16(got, exp), (c, _describe(got, exp))


# ---------------------------------------------------------------------------
# shared inputs of the fold tests: x = +-2^-3 * U(0, 1), weights 1..40
# ---------------------------------------------------------------------------
def _rows(seed, N, P):
    rng = np.random.default_rng(seed)
    return ((rng.random((N, P), dtype=np.float32) - 0.5) * 0.25).astype(F16)


def _weights(seed, N):
    return [int(v) for v in np.random.default_rng(seed + 1000).integers(1, 41, N)]


def _scores(seed, N, R=10):
    return [(int(r) + 1) / (R + 1) for r in np.random.default_rng(seed + 2000).integers(R - 2, R + 1, N)]


def _meaningful(exp) -> None:
    """Parity is never satisfied by inf == inf: the expected output is finite
    everywhere and holds a normal (subnormal-free) nonzero value."""
    e = np.concatenate([np.asarray(x, dtype=F16).ravel() for x in (exp if isinstance(exp, list) else [exp])])
    assert np.isfinite(e).all()
    assert (np.abs(e.astype(np.float32)) >= 2.0 ** -14).any()


def _factors(w, s):
    a = np.array([_half(v) for v in w], F16)
    return a, (None if s is None else np.array([_half(v) for v in s], F16)), _half(sum(w))


# ---------------------------------------------------------------------------
# 2. every vector form at a shape with full tiles, partial-tile octets and a tail
# ---------------------------------------------------------------------------
P_FORMS = 2 * 16384 + 8 * 300 + 5  # two full tiles of the widest form (8 octets x 256 lanes), 300 octets, 5 columns


@pytest.mark.parametrize("N", [1, 2, 9, 17, 18, 33])
def test_every_form_matches_numpy(dev, N):
    """Every form of fa_fedavg_f16_form, FedAvg and scored, at two row pitches.
    N: the remainder after the first row is empty, partial or full for row
    groups of 2, 4, 8 and 16.  The vector forms need rows of whole octets, and
    P + 8k never is one at this P (P % 8 == 5): the second pitch is P rounded
    up to 8 plus 8 (no multiple of 64); the pitch P + 8 itself runs through
    fa_fedavg_f16, which takes the column kernel there."""
    from fedlesscan_amd import _lib
    B = _lib.load_bench()
    P = P_FORMS
    X = _rows(N, N, P)
    w, sc = _weights(N, N), _scores(N, N)
    exp = {False: _oracle(X, w), True: _oracle(X, w, sc)}
    for e in exp.values():
        assert e.dtype == F16
        _meaningful(e)
    nforms = B.fa_num_f16_forms()
    assert nforms >= 11
    for ldx in ((P + 63) // 64 * 64, (P + 7) // 8 * 8 + 8):
        Xp = np.zeros((N, ldx), F16)
        Xp[:, :P] = X
        Xd = _dev_bits(Xp, dev)
        for scored in (False, True):
            a, s, d = _factors(w, sc if scored else None)
            for form in range(nforms):
                got = _raw(dev, Xd, P, a, s, d, form)
                assert same_bits16(got, exp[scored]), (B.fa_f16_form_name(form).decode(), N, ldx, scored,
                                                       _describe(got, exp[scored]))
    Xp = np.zeros((N, P + 8), F16)
    Xp[:, :P] = X
    for scored in (False, True):
        a, s, d = _factors(w, sc if scored else None)
        got = _raw(dev, _dev_bits(Xp, dev), P, a, s, d)
        assert same_bits16(got, exp[scored]), ("pitch P + 8", N, scored, _describe(got, exp[scored]))


def test_every_form_at_its_smallest_three_piece_shape(dev):
    """Every form of fa_fedavg_f16_form at the smallest P with all three column
    pieces of its tiling: one full tile of 256 * C octets, a last tile with
    exactly one octet, and a 3-column tail.  N = 1 (the first row alone), 2 (no
    full row group) and U + 2 (one group of U rows and a leftover row)."""
    import re
    from fedlesscan_amd import _lib
    B = _lib.load_bench()
    exp = {}
    for form in range(B.fa_num_f16_forms()):
        name = B.fa_f16_form_name(form).decode()
        U, C = map(int, re.search(r"u(\d+)c(\d+)$", name).groups())
        P = 256 * C * 8 + 8 + 3
        for N in (1, 2, U + 2):
            X = _rows(7 * N + C, N, P)
            w, sc = _weights(N, N), _scores(N, N)
            Xp = np.zeros((N, (P + 7) // 8 * 8), F16)
            Xp[:, :P] = X
            Xd = _dev_bits(Xp, dev)
            for scored in (False, True):
                if (N, P, scored) not in exp:
                    exp[N, P, scored] = _oracle(X, w, sc if scored else None)
                    _meaningful(exp[N, P, scored])
                a, s, d = _factors(w, sc if scored else None)
                got = _raw(dev, Xd, P, a, s, d, form)
                assert same_bits16(got, exp[N, P, scored]), (name, N, P, scored, _describe(got, exp[N, P, scored]))


# ---------------------------------------------------------------------------
# 3. the column kernel: odd pitch, X off 16-B alignment, out off 16-B alignment
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["odd_ldx", "x_offset", "out_offset"])
@pytest.mark.parametrize("scored", [False, True])
def test_scalar_fallback(dev, case, scored):
    from fedlesscan_amd import engine
    N, P = 5, 2053
    X = _rows(3, N, P)
    w, sc = _weights(3, N), (_scores(3, N) if scored else None)
    exp = _oracle(X, w, sc)
    _meaningful(exp)
    ldx = 2055 if case == "odd_ldx" else 2056
    x0 = 1 if case == "x_offset" else 0
    o0 = 1 if case == "out_offset" else 0
    base = torch.zeros((N, ldx), dtype=torch.float16, device=dev)
    Xd = base[:, x0:x0 + P]
    Xd.copy_(_dev_bits(X, dev))
    obase = torch.full((P + 8,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)
    out = obase[o0:o0 + P]
    assert Xd.data_ptr() % 16 == 2 * x0 and out.data_ptr() % 16 == 2 * o0
    got = engine.fold_stacked(Xd, w, sc, out=out)
    assert got is out and got.dtype == torch.float16
    assert same_bits16(_host(got), exp), (case, _describe(_host(got), exp))
    rest = _host(obase).view(np.uint16)
    assert (rest[:o0] == SENTINEL).all() and (rest[o0 + P:] == SENTINEL).all()  # nothing written outside out


# ---------------------------------------------------------------------------
# 4. in place: out is row 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ldx_pad", [0, 3])  # the vector path, the column kernel
def test_in_place_over_row0(dev, ldx_pad):
    from fedlesscan_amd import engine
    N, P = 9, P_FORMS
    X = _rows(4, N, P)
    w, sc = _weights(4, N), _scores(4, N)
    exp = _oracle(X, w, sc)
    _meaningful(exp)
    ldx = (P + 63) // 64 * 64 + ldx_pad
    base = torch.zeros((N, ldx), dtype=torch.float16, device=dev)
    base[:, :P].copy_(_dev_bits(X, dev))
    out = base[0, :P]
    got = engine.fold_stacked(base[:, :P], w, sc, out=out)
    assert got.data_ptr() == base.data_ptr()
    assert same_bits16(_host(got), exp), _describe(_host(got), exp)
    assert same_bits16(_host(base[1:, :P]), X[1:])  # the other rows untouched


# ---------------------------------------------------------------------------
# 5. one case per branch of the shape policy, each at the branch's smallest P
#    with the smallest N the branch admits
# ---------------------------------------------------------------------------
POLICY = [
    ("f16_tile_u8c1", 1, 1),                      # fewer than 1000 blocks of two octets per lane
    ("f16_tile_u8c2", 1, 1000 * 2 * 256 * 8),     # 1000 blocks of 2 octets per lane
    ("f16_tile_u4c4", 1, 1000 * 4 * 256 * 8),     # 1000 blocks of 4
    ("f16_tile_u2c8", 1, 1000 * 8 * 256 * 8),     # 1000 blocks of 8
    ("f16_bands4_u8c2", 128, (1 << 17) * 8),      # 128+ clients from 2^17 octets
    ("f16_bands4_u8c4", 128, 368000 * 8),         # 128+ clients, 368000-700000 octets
    ("f16_bands2_u2c8", 1, (1 << 22) * 8),        # 2^22 octets and more
]


PERIOD = 40009  # prime: no tile, band or pitch is a multiple of it


@pytest.mark.parametrize("name,N,P", POLICY)
def test_policy_path(dev, name, N, P):
    """The static policy's form for the shape (tuner off), through
    engine.fold_stacked.  Columns are independent, so the rows repeat a block
    of PERIOD random columns and the oracle folds that block once: column c
    must equal the oracle's column c % PERIOD.  No tile or band boundary falls
    on a multiple of the period, so a column read or written at another tile's
    or band's offset still shows."""
    from fedlesscan_amd import _lib, engine
    L = _lib.load()
    Q = min(P, PERIOD)
    Xs = _rows(5, N, Q)
    w, sc = _weights(5, N), _scores(5, N)
    ldx = (P + 63) // 64 * 64
    reps = (P + Q - 1) // Q
    Xd = torch.zeros((N, ldx), dtype=torch.float16, device=dev)
    Xd[:, :P].copy_(_dev_bits(Xs, dev).repeat(1, reps)[:, :P])
    prev = L.fa_set_autotune(0)
    try:
        st = torch.cuda.current_stream(dev).cuda_stream
        for scored in (False, True):
            assert L.fa_fold_form(4, N, P, ldx, int(scored), st).decode() == name
            s = sc if scored else None
            got = _host(engine.fold_stacked(Xd[:, :P], w, s))
            exp = _oracle(Xs, w, s)
            _meaningful(exp)
            exp = np.tile(exp, reps)[:P]
            assert same_bits16(got, exp), (name, scored, _describe(got, exp))
    finally:
        L.fa_set_autotune(prev)


def test_tuned_path_same_bits(dev):
    """With the tuner on, the first call of a shape runs every candidate form
    into the output and later calls the measured one: the same bits each time,
    and the decision is a float16 form, a kind apart from the bf16 records."""
    from fedlesscan_amd import _lib, engine
    L = _lib.load()
    N, P = 17, P_FORMS
    ldx = (P + 63) // 64 * 64
    X = _rows(6, N, P)
    w = _weights(6, N)
    exp = _oracle(X, w)
    Xp = np.zeros((N, ldx), F16)
    Xp[:, :P] = X
    Xd = _dev_bits(Xp, dev)[:, :P]
    prev = L.fa_set_autotune(1)
    try:
        for _ in range(3):
            got = _host(engine.fold_stacked(Xd, w))
            assert same_bits16(got, exp), _describe(got, exp)
        torch.cuda.synchronize()
        st = torch.cuda.current_stream(dev).cuda_stream
        assert L.fa_autotune_pending() == 0
        assert L.fa_fold_form(4, N, P, ldx, 0, st).decode().startswith("f16_")
        assert L.fa_fold_form(2, N, P, ldx, 0, st).decode().startswith("bf16_")  # a bf16 shape never reads it
    finally:
        L.fa_set_autotune(prev)


# ---------------------------------------------------------------------------
# 6. the public interface, each against the oracle's matching function
# ---------------------------------------------------------------------------
SHAPES = [(5, 5, 3), (64,), (), (33, 7)]  # includes a 0-d layer; 75 + 64 + 1 + 231 = 371 columns


def _model(seed, N, shapes=SHAPES, mixed=False):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        layers = [((rng.random(s, dtype=np.float32) - 0.5) * 0.25).astype(F16) for s in shapes]
        if mixed:
            layers.insert(1, rng.standard_normal((6, 4)).astype(np.float32))
        out.append(layers)
    return out


def _layers_equal(got, exp) -> None:
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g = g if isinstance(g, np.ndarray) else np.asarray(g)
        assert g.dtype == e.dtype and g.shape == np.shape(e), (g.dtype, e.dtype, g.shape, np.shape(e))
        if e.dtype == F16:
            assert same_bits16(g, np.asarray(e)), _describe(g.ravel(), np.asarray(e).ravel())
        else:
            import golden_cases as G
            assert G.same_bits(g, np.asarray(e))


def _f16_layers(layers):
    return [x for x in layers if x.dtype == F16]


def test_fedavg_aggregator_numpy_layers(dev):
    from fedlesscan_amd import FedAvgAggregator
    for mixed in (False, True):
        params, w = _model(7, 9, mixed=mixed), _weights(7, 9)
        with np.errstate(all="ignore"):
            exp = O.fedavg_literal(params, w)
        _meaningful(_f16_layers(exp))
        got = FedAvgAggregator()._aggregate(params, w)
        assert all(isinstance(g, np.ndarray) for g in got)
        assert [g.dtype for g in got] == [e.dtype for e in exp]
        _layers_equal(got, exp)


def test_fedavg_aggregator_cuda_tensors(dev):
    from fedlesscan_amd import FedAvgAggregator
    params, w = _model(8, 9), _weights(8, 9)
    exp = O.fedavg_literal(params, w)
    _meaningful(exp)
    tens = [[_dev_bits(x, dev).reshape(x.shape) for x in layers] for layers in params]
    got = FedAvgAggregator()._aggregate(tens, w)
    assert all(isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float16 for g in got)
    _layers_equal([_host(g.contiguous()).reshape(tuple(g.shape)) for g in got], exp)


def _npz_results(params, cards):
    from fedlesscan_amd.common.models import (ClientResult, NpzWeightsSerializerConfig, SerializedParameters,
                                              WeightsSerializerConfig)
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    cfg = WeightsSerializerConfig(type="npz", params=NpzWeightsSerializerConfig())
    return [ClientResult(parameters=SerializedParameters(blob=NpzWeightsSerializer().serialize(p), serializer=cfg),
                         cardinality=c) for p, c in zip(params, cards)]


def _dict_results(params, cards):
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    return [{"blob": NpzWeightsSerializer().serialize(p), "cardinality": c} for p, c in zip(params, cards)]


def _feats(seed, N, R=10):
    return [{"round_id": int(r)} for r in np.random.default_rng(seed + 3000).integers(R - 2, R + 1, N)]


def test_stall_aware_aggregate_from_npz(dev):
    from fedlesscan_amd import StallAwareAggregator
    from fedlesscan_amd.common.models import AggregationHyperParams
    N, R = 5, 10
    params, w, feats = _model(9, N), _weights(9, N), _feats(9, N)
    exp, _ = O.aggregate_stall_aware(_dict_results(params, w), feats, R)
    _meaningful(exp)
    got, _ = StallAwareAggregator(R, AggregationHyperParams(tolerance=2)).aggregate(_npz_results(params, w), feats)
    _layers_equal(got, exp)


@pytest.mark.parametrize("chunk", [1, 2])
def test_stream_variants_from_npz(dev, chunk):
    """The stream variants feed the float16 running aggregate back as row 0
    with the weight seen so far, as the oracle's aggregate_stream_* do."""
    from fedlesscan_amd import StreamFedAvgAggregator, StreamStallAwareAggregator
    from fedlesscan_amd.common.models import AggregationHyperParams
    N, R = 5, 10
    params, w, feats = _model(10, N), _weights(10, N), _feats(10, N)
    exp, _ = O.aggregate_stream_fedavg(_dict_results(params, w), chunk_size=chunk)
    _meaningful(exp)
    got, _ = StreamFedAvgAggregator(chunk_size=chunk).aggregate(iter(_npz_results(params, w)), feats)
    _layers_equal(got, exp)
    exp, _ = O.aggregate_stream_stall_aware(_dict_results(params, w), feats, R, chunk_size=chunk)
    _meaningful(exp)
    got, _ = StreamStallAwareAggregator(R, AggregationHyperParams(tolerance=2), chunk_size=chunk).aggregate(
        iter(_npz_results(params, w)), feats)
    _layers_equal(got, exp)


def test_handler_saves_float16_npz(dev):
    from fedlesscan_amd.common.models import NpzWeightsSerializerConfig, WeightsSerializerConfig
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    from fedlesscan_amd.handler import default_aggregation_handler
    from fedlesscan_amd.store import InMemoryClientResultStore, InMemoryParameterStore
    N = 5
    params, w = _model(11, N), _weights(11, N)
    st, ps = InMemoryClientResultStore(), InMemoryParameterStore()
    for i, r in enumerate(_npz_results(params, w)):
        st.save("s", 3, f"c{i}", r)
    cfg = WeightsSerializerConfig(type="npz", params=NpzWeightsSerializerConfig())
    res = default_aggregation_handler("s", 3, st, ps, cfg)
    assert res.new_round_id == 4 and res.num_clients == N
    saved = NpzWeightsSerializer().deserialize(ps.load("s", 4).blob)
    exp, _ = O.aggregate_fedavg(_dict_results(params, w))
    _meaningful(exp)
    assert all(x.dtype == F16 for x in saved)
    _layers_equal(saved, exp)


# ---------------------------------------------------------------------------
# 7. the reference's overflow behaviour is kept
# ---------------------------------------------------------------------------
def test_reference_overflow_kept(dev):
    """Cardinalities summing above 65504, exactly as numpy computes them:
    70000 rounds to inf (x * inf is +-inf, 0 * inf NaN) and so does the total
    110002 (inf / inf NaN); 70008 rounds to inf under finite sums (all zeros);
    65519 rounds DOWN to 65504 and stays finite, so a product that overflowed
    stays inf; 2049 rounds to 2048."""
    from fedlesscan_amd import FedAvgAggregator, engine
    N, P = 4, 4099
    X = _rows(12, N, P)
    X[:, :64] = 0  # zeros under an infinite weight
    X[0, 64:128] = F16(-0.0)
    X[0, 128:192] = F16(2.0)  # 2 * 40000 and 2 * 65000 overflow
    Xd = _dev_bits(X, dev)
    seen = {"nan": False, "zero": False, "inf": False}
    for w in ([70000, 1, 2049, 37952], [40000, 30000, 3, 5], [65000, 400, 100, 19]):
        assert sum(w) > 65504
        exp = _oracle(X, w)
        got = _host(engine.fold_stacked(Xd, w))
        assert exp.dtype == F16 and same_bits16(got, exp), (w, _describe(got, exp))
        seen["nan"] |= bool(np.isnan(exp).any())
        seen["zero"] |= bool((exp == 0).any())
        seen["inf"] |= bool(np.isinf(exp).any())
    assert all(seen.values()), seen
    w = [70000, 1, 2049, 37952]
    params = [[X[i, :100].reshape(10, 10), X[i, 100:]] for i in range(N)]
    with np.errstate(all="ignore"):
        expl = O.fedavg_literal(params, w)
    _layers_equal(FedAvgAggregator()._aggregate(params, w), expl)


# ---------------------------------------------------------------------------
# 8. numpy-scalar weights promote the fold
# ---------------------------------------------------------------------------
def test_numpy_scalar_weights_promote(dev):
    import golden_cases as G
    from fedlesscan_amd import FedAvgAggregator, engine
    N, P = 7, 1029
    X = _rows(13, N, P)
    w32 = [np.float32(v) for v in _weights(13, N)]
    exp = O.fedavg_stacked(X, w32)
    assert exp.dtype == np.float32
    got = engine.fold_stacked(_dev_bits(X, dev), w32)
    assert got.dtype == torch.float32 and G.same_bits(got.cpu().numpy(), exp)
    params = [[X[i, :29], X[i, 29:].reshape(10, 100)] for i in range(N)]
    expl = O.fedavg_literal(params, w32)  # host float16 layers get past the stacking
    gotl = FedAvgAggregator()._aggregate(params, w32)
    assert [g.dtype for g in gotl] == [np.float32, np.float32]
    assert all(G.same_bits(g, e) for g, e in zip(gotl, expl))
    w64 = [np.float64(v) for v in _weights(13, N)]
    got = engine.fold_stacked(_dev_bits(X, dev), w64)
    exp = O.fedavg_stacked(X, w64)
    assert got.dtype == torch.float64 and G.same_bits(got.cpu().numpy(), exp)


# ---------------------------------------------------------------------------
# the branch's own checks
# ---------------------------------------------------------------------------
def test_out_is_checked_and_capture_refused(dev):
    from fedlesscan_amd import engine
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    X = _dev_bits(_rows(14, 3, 40), dev)
    w = [1, 2, 3]
    with pytest.raises(ValueError):
        engine.fold_stacked(X, w, out=torch.empty(40, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        engine.fold_stacked(X, w, out=torch.empty(39, dtype=torch.float16, device=dev))
    with pytest.raises(ValueError):
        engine.fold_stacked(X, w, out=torch.empty(80, dtype=torch.float16, device=dev)[::2])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(InvalidParameterShapeError, match="capture"):
        with torch.cuda.graph(g, stream=side):
            engine.fold_stacked(X, w)
    torch.cuda.synchronize()
    out = engine.fold_stacked(X, w)  # the device is fine afterwards
    assert same_bits16(_host(out), _oracle(_host(X), w))
