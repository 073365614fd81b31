"""Device-side aggregation engine: numpy-exact scalar factors + HIP folds.

Layering
  engine.fold_stacked(X, weights, scores)   X: CUDA tensor [N, P] (row pitch = X.stride(0))
  engine.fold_rows(rows, weights, scores)   N separately allocated CUDA rows (pointer list: fp32,
                                            bf16, float16, float64, int32, int64; engine.RowSet prepares a
                                            reusable row set)
  engine.aggregate_layers(params, weights)  host or device per-client layer lists -> per-layer outputs

The scalar factors are formed on the host exactly as numpy forms them in the
reference (fed_avg_aggregator.py:31-41, stall_aware_aggregation.py:52-66):
Python-scalar weights are *weak* (rounded once to the array dtype), the total
is a Python ``sum`` (exact for ints), scores are Python floats from a double
division.  The kernels then fold in client order with separate roundings.
Which dtype numpy gives every product, running sum and the quotient is decided
in one place, fold_plan: a fold of one dtype throughout runs in one uniform
kernel, any other is folded term by term as numpy types it (_fold_general).

There is no CPU fallback anywhere in this module: every output element is
computed by libfedavg_hip.so on the GPU, or the call raises.
"""
from __future__ import annotations

import ctypes
import functools
import operator
import os
import threading
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .aggregator.exceptions import InvalidParameterShapeError

_TORCH_TO_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32,
                torch.int64: np.int64, torch.float16: np.float16}
_NP_TO_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
                np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
                np.dtype(np.float16): torch.float16}
ROW_ALIGN = 64  # elements; row pitch multiple of 256 B for fp32
# the OCP fp8 dtypes the library folds from the bytes themselves -> fa_fedavg_fp8's fmt
_FP8_FORMATS = {torch.float8_e4m3fn: _lib.FA_FP8_E4M3FN, torch.float8_e5m2: _lib.FA_FP8_E5M2}


class ScaledLayer(NamedTuple):
    """A client's fp8 layer with its dequantisation scale, as aggregate_layers
    (and the strategy classes' _aggregate) take it: the layer counts as
    q.to(float32) * np.float32(scale).  Every client wraps a layer or none does."""
    q: torch.Tensor
    scale: float


# the MX element dtypes (one E8M0 scale byte per 32 flat elements) -> fa_fedavg_mx's fmt
_MX_FORMATS = {torch.float8_e4m3fn: _lib.FA_MX_E4M3, torch.float8_e5m2: _lib.FA_MX_E5M2,
               torch.float4_e2m1fn_x2: _lib.FA_MX_E2M1}
_MX_SCALE_DTYPES = (torch.uint8, torch.float8_e8m0fnu)
# float4_e2m1fn_x2 rows whose block scales have this dtype are NVFP4: one e4m3fn scale byte per 16 flat elements
_NVFP4_SCALE_DTYPE = torch.float8_e4m3fn
_SCALE_BYTES_MSG = "E8M0 bytes (float8_e8m0fnu or uint8; float8_e4m3fn with float4_e2m1fn_x2 rows: NVFP4)"


def _is_nvfp4(e) -> bool:
    return isinstance(e, torch.Tensor) and e.dtype == _NVFP4_SCALE_DTYPE


def _block_scale_kind(dt: torch.dtype, e, what: str) -> int:
    """The elements per scale byte of rows of dtype dt with the block scales e:
    32 (MX, E8M0 bytes) or 16 (NVFP4, e4m3fn bytes with float4 rows)."""
    if _is_nvfp4(e):
        if dt != torch.float4_e2m1fn_x2:
            raise InvalidParameterShapeError(f"{what}: float8_e4m3fn block scales are NVFP4's and go with "
                                             f"float4_e2m1fn_x2 rows, got {dt} rows")
        return _lib.FA_NVFP4_BLOCK
    if not (isinstance(e, torch.Tensor) and e.dtype in _MX_SCALE_DTYPES):
        raise InvalidParameterShapeError(f"{what} must hold {_SCALE_BYTES_MSG}, got {getattr(e, 'dtype', type(e))}")
    return 32


class MXLayer(NamedTuple):
    """A client's MX block-scaled layer, as aggregate_layers (and the strategy
    classes' _aggregate) take it: q the elements (float8_e4m3fn, float8_e5m2, or
    float4_e2m1fn_x2 with two columns per byte, the even one in the low nibble),
    e the E8M0 scale bytes (uint8 or float8_e8m0fnu), one per 32 elements of the
    FLATTENED layer (ceil(size / 32) of them, a last partial block allowed: a
    layer whose last dimension is a multiple of 32 is in the standard MX layout
    along it), scale an optional dequantisation scale of the whole tensor (as
    ScaledLayer's).  The layer counts as upcast(q) * 2^(e - 127) [* scale]; the
    result has q's shape, the last dimension doubled for float4.  Every client
    wraps a layer, in one format, or none does.
    NVFP4: q float4_e2m1fn_x2 and e of dtype float8_e4m3fn, one scale byte per
    16 elements of the flattened layer (ceil(size / 16)), scale the tensor's
    float32 scale: the layer counts as upcast(q) * float32(e) [* scale]
    (fa_fedavg_nvfp4_ptrs, a fold per layer)."""
    q: torch.Tensor
    e: torch.Tensor
    scale: Optional[float] = None


def _mx_cols(dt: torch.dtype, nbytes: int) -> int:
    return 2 * nbytes if dt == torch.float4_e2m1fn_x2 else nbytes


def default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("fedlesscan_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def result_dtype(in_dtype: np.dtype, weights: Sequence, scores: Optional[Sequence] = None,
                 total=None) -> np.dtype:
    """dtype numpy gives `reduce(add, [x * n_i (* s_i)]) / sum(n)` (NEP 50 weak Python scalars).
    The result's dtype only: fold_plan says how numpy gets there.  The routes ask it
    whether a float32 / float16 fold stays in its dtype (then the plan is uniform too)."""
    in_dtype = np.dtype(in_dtype)
    if in_dtype.kind == "f":
        # Python bool / int / float scalars are weak: a float array keeps its dtype
        kinds = set(map(type, weights))
        if scores is not None:
            kinds.update(map(type, scores))
        if total is not None:
            kinds.add(type(total))
        if kinds <= {bool, int, float}:
            return in_dtype
    if total is None:
        total = sum(weights)
    dt = np.result_type(in_dtype, *weights, *(scores or ()), total)
    if dt.kind in "iu" or dt.kind == "b":
        dt = np.result_type(dt, np.float64)  # true_divide of integers
    return dt


_WEAK = (bool, int, float)
_F16, _F32, _F64 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)
_I32_MIN, _I32_END = -2 ** 31, 2 ** 31
_I63 = 2 ** 63


class FoldPlan(NamedTuple):
    """The dtypes numpy gives every step of `reduce(add, [layer_i * n_i (* s_i)]) / total`.

    prod[i]   dtype of `layer_i * n_i`
    term[i]   dtype of the finished term (`* s_i` applied; prod[i] without scores)
    acc[i]    dtype of the running sum once term i is in it (acc[0] is term[0])
    quot      dtype of the quotient (None when no row is folded)
    uniform   the one compute dtype of a fold the uniform kernels do -- every
              row widened once to it, every product, sum and the quotient in it
              (an integer fold divides into float64) -- else None."""
    prod: tuple
    term: tuple
    acc: tuple
    quot: Optional[np.dtype]
    uniform: Optional[np.dtype]


def _scalar_key(x):
    """What decides the dtype numpy gives `array (op) x`, as a hashable key:
    the type of a weak Python scalar, the dtype of a numpy scalar.  None where
    the value itself matters (a Python int that some integer dtype cannot hold
    raises OverflowError, a huge one does on a float array) or for any other
    object: numpy is then asked with the value."""
    t = type(x)
    if t is float or t is bool:
        return t
    if t is int:
        return int if _I32_MIN <= x < _I32_END else None
    if isinstance(x, np.generic) and x.dtype.kind in "biuf":
        return x.dtype
    return None


@functools.lru_cache(maxsize=None)
def _op_dtype_keyed(op, dt, key):
    x = key(1) if isinstance(key, type) else key.type(1)
    return op(np.empty(0, dt), x).dtype


def _op_dtype(op, dt, x):
    """dtype of op(array of dtype dt, scalar x): numpy itself, on a zero-length
    array, so it also raises what numpy raises."""
    key = _scalar_key(x)
    if key is not None:
        return _op_dtype_keyed(op, dt, key)
    with np.errstate(all="ignore"):  # a Python int beyond a float dtype's range becomes inf, as in the fold
        return op(np.empty(0, dt), x).dtype


@functools.lru_cache(maxsize=None)
def _add_dtype(a, b):
    return np.add(np.empty(0, a), np.empty(0, b)).dtype


def fold_plan(row_dtypes, weights: Sequence, scores: Optional[Sequence] = None, total=None) -> FoldPlan:
    """The promotion plan of one fold, asked of numpy on zero-length arrays
    (NEP 50: every product is typed on its own, a Python number is weak, a
    numpy scalar is not).  Pure host code.  row_dtypes: one dtype for every
    row, or one per row (the stream variants put their float64 running model
    ahead of the clients' rows).  zip() truncation over rows, weights and
    scores is kept; `total` defaults to the sum of ALL weights.  Raises what
    the reference's expression raises (OverflowError for a Python int an
    integer layer cannot hold)."""
    n = min(len(weights), len(scores) if scores is not None else len(weights))
    if isinstance(row_dtypes, (list, tuple)):
        n = min(n, len(row_dtypes))
        rows = [np.dtype(d) for d in row_dtypes[:n]]
    else:
        rows = [np.dtype(row_dtypes)] * n
    if total is None:
        total = sum(weights)
    if n and rows[0].kind == "f" and rows.count(rows[0]) == n:
        # float rows under weak Python numbers keep their dtype throughout
        vals = [*weights[:n], total] if scores is None else [*weights[:n], *scores[:n], total]
        if set(map(type, vals)) <= set(_WEAK) and all(type(v) is not int or -_I63 <= v < _I63 for v in vals):
            same = (rows[0],) * n
            return FoldPlan(same, same, same, rows[0], rows[0] if rows[0] in _NP_TO_TORCH else None)
    prod, term, acc = [], [], []
    for i in range(n):
        p = _op_dtype(np.multiply, rows[i], weights[i])
        t = p if scores is None else _op_dtype(np.multiply, p, scores[i])
        prod.append(p)
        term.append(t)
        acc.append(t if not acc else _add_dtype(acc[-1], t))
    if not n:
        return FoldPlan((), (), (), None, None)
    quot = _op_dtype(np.true_divide, acc[-1], total)
    c = acc[-1]
    uniform = c if (c in _NP_TO_TORCH and quot == (c if c.kind == "f" else _F64)
                    and all(r in _NP_TO_TORCH for r in rows)
                    and prod.count(c) == n and term.count(c) == n and acc.count(c) == n) else None
    return FoldPlan(tuple(prod), tuple(term), tuple(acc), quot, uniform)


_EXACT_F64 = float(2 ** 53)


def _load_hostfast():
    """The optional CPython helper built next to the HIP libraries (hostfast.c);
    None when it is absent (the numpy path below gives the same bits)."""
    if not os.path.exists(_lib.HOSTFAST_PATH):
        return None
    from importlib.util import module_from_spec, spec_from_file_location
    spec = spec_from_file_location("_hostfast", _lib.HOSTFAST_PATH)
    mod = module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_hostfast = _load_hostfast()


def weak_f32(values) -> Optional[np.ndarray]:
    """np.float32 roundings of `values` when every item is exactly a Python
    bool, int (|v| < 2**53) or float -- numpy's weak scalars, which keep a
    float32 fold float32 -- in one C loop; None otherwise (or without the
    helper), for the general path: result_dtype + round_scalars."""
    if _hostfast is None:
        return None
    b = _hostfast.round_weak_f32(values)
    return None if b is None else np.frombuffer(b, dtype=np.float32)


def round_scalars(values: Sequence, dt: np.dtype) -> np.ndarray:
    """[dt(v) for v in values] -- numpy's rounding of Python (or numpy) scalars
    to `dt`, vectorised.  Going through float64 first is exact whenever every
    value is representable there (ints below 2**53, any float), so rounding the
    float64 array once gives the same bits as rounding each scalar; anything
    else takes the per-element loop."""
    dt = np.dtype(dt)
    try:
        v = (values.astype(np.float64) if isinstance(values, np.ndarray)
             else np.fromiter(values, dtype=np.float64, count=len(values)))
    except (TypeError, ValueError, OverflowError):
        v = None
    if v is not None and v.ndim == 1 and dt.kind == "f" and not (v.size and np.abs(v).max() >= _EXACT_F64):
        return v.astype(dt)
    return np.array([dt.type(x) for x in values], dtype=dt)


class _FactorRing:
    """Page-locked staging slots for the per-client factors of one device: the
    factors of a call travel in ONE async H2D on the caller's stream (instead
    of synchronous pageable copies).  A slot is rewritten only after the copy
    that last read it has completed (its event)."""

    SLOTS, SLOT_BYTES = 8, 1 << 17

    def __init__(self):
        self.host = [torch.empty(self.SLOT_BYTES, dtype=torch.uint8, pin_memory=True) for _ in range(self.SLOTS)]
        self.done = [None] * self.SLOTS
        self.k = 0
        self.lock = threading.Lock()  # callers on several threads share the ring

    def stage(self, parts: List[np.ndarray], dev: torch.device) -> List[torch.Tensor]:
        nbytes = sum(p.nbytes for p in parts)
        if nbytes > self.SLOT_BYTES:  # very many clients: plain copies
            return [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in parts]
        with self.lock:
            k = self.k
            self.k = (k + 1) % self.SLOTS
            if self.done[k] is not None:
                self.done[k].synchronize()
            hv = self.host[k].numpy()
            off = 0
            for p in parts:
                hv[off:off + p.nbytes] = np.ascontiguousarray(p).view(np.uint8).reshape(-1)
                off += p.nbytes
            d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            d.copy_(self.host[k][:nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            self.done[k] = ev
        out, off = [], 0
        for p in parts:
            out.append(d[off:off + p.nbytes].view(_NP_TO_TORCH[p.dtype]))
            off += p.nbytes
        return out


_rings: dict = {}
_rings_lock = threading.Lock()


def stage_factors(parts: List[np.ndarray], dev: torch.device) -> List[torch.Tensor]:
    ring = _rings.get(dev)
    if ring is None:
        with _rings_lock:
            ring = _rings.setdefault(dev, None) or _FactorRing()
            _rings[dev] = ring
    return ring.stage(parts, dev)


class Factors:
    """a_i, s_i and the divisor as numpy would round them for compute dtype `dt`."""

    def __init__(self, weights: Sequence, scores: Optional[Sequence], dt: np.dtype, int_weights=False,
                 total=None):
        self.total = sum(weights) if total is None else total
        if int_weights:
            self.a = np.asarray([int(w) for w in weights], dtype=np.int64)
            self.div = float(self.total)
        else:
            self.a = round_scalars(weights, dt)
            self.div = np.dtype(dt).type(self.total)
        self.s = None if scores is None else round_scalars(scores, dt)

    @classmethod
    def weak_f32(cls, weights: Sequence, scores: Optional[Sequence], total=None) -> Optional["Factors"]:
        """Factors of a float32 fold whose weights, scores and total are all
        weak Python scalars (the reference's cardinalities and scores are):
        the result dtype is float32 without a type scan and the rounding is
        one C loop.  None when any value is something else."""
        if total is not None and type(total) not in (bool, int, float):
            return None
        a = weak_f32(weights)
        if a is None:
            return None
        s = None
        if scores is not None:
            s = weak_f32(scores)
            if s is None:
                return None
        f = cls.__new__(cls)
        f.total = sum(weights) if total is None else total
        f.a, f.s = a, s
        f.div = np.float32(f.total)
        return f

    def host(self):
        """(a, s) as host addresses for the *_hostf entries (s: None)."""
        return self.a.ctypes.data, (None if self.s is None else self.s.ctypes.data)

    def to(self, device):
        parts = [self.a] if self.s is None else [self.a, self.s]
        staged = stage_factors(parts, device)
        return staged[0], (staged[1] if self.s is not None else None)


def _captured_factors(f: Factors, dev) -> tuple:
    """Under a HIP graph capture: the float32 factors (a, s or None) in a
    tensor allocated inside the capture -- memory the graph owns -- written by
    fill kernels that carry the values in their arguments (fa_factors_fill),
    for the device-factor entries; the _hostf entries refuse capture."""
    n = len(f.a)
    buf = torch.empty(n * (1 if f.s is None else 2), dtype=torch.float32, device=dev)
    _lib.call("fa_factors_fill", buf.data_ptr(), *f.host(), n, stream_ptr(dev))
    return buf[:n], (None if f.s is None else buf[n:])


# fa_fedavg_widen's kinds (include/fedavg_hip.h, FA_WIDEN_*): (row dtype, fold dtype) -> kind
_WIDEN_KINDS = {(_F16, _F32): _lib.FA_WIDEN_F16_F32, (_F16, _F64): _lib.FA_WIDEN_F16_F64,
                (_F32, _F64): _lib.FA_WIDEN_F32_F64, (np.dtype(np.int32), _F64): _lib.FA_WIDEN_I32_F64,
                (np.dtype(np.int64), _F64): _lib.FA_WIDEN_I64_F64,
                (np.dtype(np.int32), np.dtype(np.int64)): _lib.FA_WIDEN_I32_I64}


def widen_kind(in_dt, dt) -> Optional[int]:
    """The fa_fedavg_widen kind that folds rows of dtype `in_dt` in the promoted
    dtype `dt` (a fold_plan's `uniform`) from the narrow rows themselves, or
    None: the fold stays in its dtype, numpy types it term by term (dt None),
    or no kernel converts that pair on load.  Pure host code."""
    if in_dt is None or dt is None:
        return None
    return _WIDEN_KINDS.get((np.dtype(in_dt), np.dtype(dt)))


def widen_enabled() -> bool:
    """FEDAVG_WIDEN=0 keeps a promoted stacked fold on the widened copy
    (X.to(wide dtype), then the wide dtype's kernel).  Read per call, so a
    process can switch it between folds."""
    return os.environ.get("FEDAVG_WIDEN", "1") != "0"


def _widen(kind: Optional[int], P: int) -> bool:
    """A promoted stacked fold reads the narrow rows (fa_fedavg_widen): a kind
    exists, there are columns, no capture is in progress (a captured fold keeps
    the route it had), and the switch is on."""
    return (kind is not None and P > 0 and widen_enabled()
            and not torch.cuda.is_current_stream_capturing())


def widen_rows_enabled() -> bool:
    """FEDAVG_WIDEN_ROWS=1 (read per call) lets aggregate_layers and the
    strategy classes fold a promoted device group through the widening row
    tables (fold_rows / fold_model_rows) instead of stacking it; the default
    keeps the stacked copy there.  fold_rows and fold_model_rows themselves
    take the tables whatever it says."""
    return os.environ.get("FEDAVG_WIDEN_ROWS", "0") == "1"


def widen_factors(in_dt, weights: Sequence, scores: Optional[Sequence] = None, total=None):
    """(kind, Factors) of a promoted fold over rows of dtype `in_dt` that a
    widening kernel computes from the narrow rows, with the factors fold_stacked
    builds for that kind (the kind's factor dtype; int64 cardinalities for
    int32 rows under int64 weights) -- or None: the fold is not promoted, numpy
    types it term by term, no kernel converts that pair, or FEDAVG_WIDEN=0.
    Pure host code; raises what fold_plan raises."""
    if not widen_enabled() or not len(weights):
        return None
    dt = fold_plan(in_dt, weights, scores, total).uniform
    kind = widen_kind(in_dt, dt)
    if kind is None:
        return None
    if dt.kind == "i":
        return kind, Factors(weights, None, dt, int_weights=True, total=total)
    return kind, Factors(weights, scores, dt, total=total)


_widen_geometries: dict = {}


def widen_geometry(kind: int) -> tuple:
    """fa_widen_geometry: (columns of a 16-byte source unit, units per lane, rows ahead).  No GPU."""
    g = _widen_geometries.get(kind)
    if g is None:
        u, c, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.call("fa_widen_geometry", kind, ctypes.addressof(u), ctypes.addressof(c), ctypes.addressof(r))
        g = _widen_geometries[kind] = (u.value, c.value, r.value)
    return g


def _widen_out_dtype(kind: int) -> torch.dtype:
    return torch.float32 if kind == _lib.FA_WIDEN_F16_F32 else torch.float64


def _check_matrix(X: torch.Tensor) -> tuple[int, int, int]:
    if not X.is_cuda:
        raise ValueError("X must be a CUDA (HIP) tensor")
    if X.dim() != 2 or X.stride(1) != 1:
        raise InvalidParameterShapeError(f"X must be 2-D with unit column stride, got {tuple(X.shape)} "
                                         f"strides {X.stride()}")
    N, P = X.shape
    return N, P, X.stride(0) if N > 1 else max(P, 1)


def fold_stacked(X: torch.Tensor, weights: Sequence, scores: Optional[Sequence] = None, *,
                 out: Optional[torch.Tensor] = None, want_bf16: bool = False, total=None,
                 exact: bool = True, out_bf16: Optional[torch.Tensor] = None, scales: Optional[Sequence] = None,
                 block_scales: Optional[torch.Tensor] = None, out_format: Optional[torch.dtype] = None,
                 out_mx=None):
    """FedAvg (scores None) / stall-aware fold over the rows of X, in row order.

    `total` overrides the divisor sum (used when zip() truncated the rows but
    the reference still divides by the sum of every weight).  Returns `out`
    ([P] tensor in the result dtype; float16 rows under Python-number factors
    give float16, every operation rounded to binary16 as numpy does).  bf16 input: want_bf16=True returns
    (out_f32, out_bf16); out_bf16= (a [P] bfloat16 tensor) receives the RNE
    copy in place -- without out it is the only output (no fp32 result is
    stored, ABI 5) and is returned alone, with out the pair is returned.
    exact=False (fp32 only) opts into the split-client fold,
    fa_fedavg_f32_splitn: faster on very narrow models, deterministic, but NOT
    bit-identical to the reference (a different association of the same sum).
    fp8 rows (float8_e4m3fn, float8_e5m2; no reference path) are upcast exactly
    and folded in float32 with the bf16 fold's outputs; scales= (N floats,
    rounded to float32 as the weights are) multiplies row i by scale_i before
    its weight, with a rounding of its own.
    MX rows: block_scales= E, [N, ceil(P / 32)] E8M0 bytes (float8_e8m0fnu or
    uint8, any pitch) with X [N, P] of float8_e4m3fn / float8_e5m2 or [N, P / 2]
    of float4_e2m1fn_x2; element p of row i counts as upcast(q) * 2^(E[i, p >>
    5] - 127), then scales= as for fp8 rows (MXLayer says the rest).
    NVFP4 rows: X [N, P / 2] of float4_e2m1fn_x2 with block_scales= E of dtype
    float8_e4m3fn, [N, ceil(P / 16)] at any pitch; element p counts as
    upcast(q) * float32(E[i, p >> 4]), scales= the tensors' float32 scales
    (fa_fedavg_nvfp4); out_format / out_mx do not go with them.
    fp8 and MX rows: out_format= (float8_e4m3fn, float8_e5m2 or
    float4_e2m1fn_x2) quantises the result to MX in the same launch
    (fa_fedavg_fp8_q / fa_fedavg_mx_q; the contract is DESIGN.md 2's) and
    returns MXLayer(q, e): q flat in that dtype, e [ceil(P / 32)]
    float8_e8m0fnu, a valid MX row of a further fold.  out_mx=(q, e) supplies
    the buffers; out= still receives the float32 result.  Not with want_bf16 /
    out_bf16, nor with rows of another dtype.
    """
    N, P, ldx = _check_matrix(X)
    if len(weights) != N or (scores is not None and len(scores) != N):
        raise InvalidParameterShapeError(f"{N} rows but {len(weights)} weights"
                                         + ("" if scores is None else f" / {len(scores)} scores"))
    dev = X.device
    if block_scales is not None or X.dtype == torch.float4_e2m1fn_x2:
        return _fold_mx(X, block_scales, None, weights, scores, scales, out, total, want_bf16, out_bf16, out_format,
                        out_mx)
    if X.dtype in _FP8_FORMATS:
        return _fold_fp8(X, None, weights, scores, scales, out, total, want_bf16, out_bf16, out_format, out_mx)
    if out_format is not None or out_mx is not None:
        raise InvalidParameterShapeError(f"out_format / out_mx are for fp8 and MX rows, got {X.dtype}")
    if scales is not None:
        raise InvalidParameterShapeError(f"scales are for fp8 rows, got {X.dtype}")
    st = stream_ptr(dev)
    if out_bf16 is not None and X.dtype != torch.bfloat16:
        raise InvalidParameterShapeError("out_bf16 is for bfloat16 rows")
    if X.dtype == torch.bfloat16:
        f = Factors.weak_f32(weights, scores, total) or Factors(weights, scores, np.dtype(np.float32), total=total)
        if out_bf16 is not None:
            if not (out_bf16.is_cuda and out_bf16.dtype == torch.bfloat16 and out_bf16.is_contiguous()
                    and out_bf16.numel() >= P):
                raise ValueError(f"out_bf16 must be a contiguous CUDA bfloat16 tensor of >= {P} elements")
            outb = out_bf16
        else:
            outb = torch.empty(P, dtype=torch.bfloat16, device=dev) if want_bf16 else None
        if out is None and (outb is None or want_bf16):
            out = torch.empty(P, dtype=torch.float32, device=dev)
        if torch.cuda.is_current_stream_capturing():
            a, s = _captured_factors(f, dev)
            _lib.call("fa_fedavg_bf16", X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s), float(f.div),
                      _ptr(out), _ptr(outb), st)
        else:
            _lib.call("fa_fedavg_bf16_hostf", X.data_ptr(), N, P, ldx, *f.host(), float(f.div),
                      _ptr(out), _ptr(outb), st)
        if want_bf16:
            return out, outb
        if out_bf16 is not None:
            return outb if out is None else (out, outb)
        return out
    in_dt = np.dtype(_TORCH_TO_NP.get(X.dtype, np.void))
    if in_dt == np.void:
        raise InvalidParameterShapeError(f"unsupported dtype {X.dtype}")
    # the common case (float32 layers, Python-number weights) skips the type scan
    fw = Factors.weak_f32(weights, scores, total) if in_dt == np.float32 else None
    if fw is not None:
        dt = _F32
    elif N == 0:
        dt = result_dtype(in_dt, weights, scores, total)
    else:
        plan = fold_plan(in_dt, weights, scores, total)
        dt = plan.uniform
        if dt is None:  # numpy types this fold term by term: no single kernel is its arithmetic
            return _fold_general([X], plan, weights, scores, total, out)
    if dt.kind == "i":
        # `layer * n` and the running sum stay in the integer dtype and wrap, the
        # quotient is float64; numpy-scalar weights may widen int32 rows to int64 first
        f = Factors(weights, None, dt, int_weights=True, total=total)
        a, _ = f.to(dev)
        if in_dt != dt:
            if _widen(widen_kind(in_dt, dt), P):  # int32 rows, int64 products: sign-extended on load
                out = out if out is not None else torch.empty(P, dtype=torch.float64, device=dev)
                _lib.call("fa_fedavg_widen", widen_kind(in_dt, dt), X.data_ptr(), N, P, ldx, a.data_ptr(), None,
                          f.div, out.data_ptr(), st)
                stats["widened_folds"] += 1
                return out
            X = X.to(_NP_TO_TORCH[dt])
            ldx = X.stride(0) if N > 1 else max(P, 1)
        out = out if out is not None else torch.empty(P, dtype=torch.float64, device=dev)
        name = "fa_fedavg_i32" if dt == np.int32 else "fa_fedavg_i64"
        _lib.call(name, X.data_ptr(), N, P, ldx, a.data_ptr(), f.div, out.data_ptr(), st)
        return out
    if dt == np.float16:
        # float16 rows under weak (Python-number) factors stay float16 in numpy:
        # binary16 products, sums and quotient (fa_fedavg_f16)
        if torch.cuda.is_current_stream_capturing():
            raise InvalidParameterShapeError("the float16 fold does not run under stream capture "
                                             "(the captured factor fill carries float32 factors only)")
        if out is None:
            out = torch.empty(P, dtype=torch.float16, device=dev)
        elif not (out.is_cuda and out.dtype == torch.float16 and out.is_contiguous() and out.numel() >= P):
            raise ValueError(f"out must be a contiguous CUDA float16 tensor of >= {P} elements")
        f = Factors(weights, scores, dt, total=total)
        a, s = f.to(dev)
        _lib.call("fa_fedavg_f16", X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s),
                  int(np.asarray(f.div, dtype=np.float16).view(np.uint16)), out.data_ptr(), st)
        return out
    if dt not in (np.float32, np.float64):
        raise InvalidParameterShapeError(f"unsupported result dtype {dt} (input {in_dt})")
    if in_dt != dt:
        # numpy promotes the operand before multiplying; same on the device: in
        # registers, right after the load (fa_fedavg_widen), or, where no kernel
        # does (and for the opt-in split fold), as a widened copy of the rows
        kind = widen_kind(in_dt, dt)
        if (exact or dt != np.float32) and _widen(kind, P):
            f = Factors(weights, scores, dt, total=total)
            out = out if out is not None else torch.empty(P, dtype=_NP_TO_TORCH[dt], device=dev)
            a, s = f.to(dev)
            _lib.call("fa_fedavg_widen", kind, X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s), float(f.div),
                      out.data_ptr(), st)
            stats["widened_folds"] += 1
            return out
        X = X.to(_NP_TO_TORCH[dt])
        ldx = X.stride(0) if N > 1 else max(P, 1)
    f = fw or Factors(weights, scores, dt, total=total)
    out = out if out is not None else torch.empty(P, dtype=_NP_TO_TORCH[dt], device=dev)
    if dt == np.float32:
        # the split-client kernel needs 16-B aligned rows; any other layout
        # takes the exact fold, which is bit-identical to the reference
        split = not exact and X.data_ptr() % 16 == 0 and ldx % 4 == 0 and out.data_ptr() % 16 == 0
        if split:
            a, s = f.to(dev)
            _lib.call("fa_fedavg_f32_splitn", X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s), float(f.div),
                      out.data_ptr(), st)
        elif torch.cuda.is_current_stream_capturing():
            a, s = _captured_factors(f, dev)
            _lib.call("fa_fedavg_f32", X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s), float(f.div),
                      out.data_ptr(), st)
        else:  # factors from host memory: the library stages them (one C call)
            _lib.call("fa_fedavg_f32_hostf", X.data_ptr(), N, P, ldx, *f.host(), float(f.div), out.data_ptr(), st)
    else:
        a, s = f.to(dev)
        _lib.call("fa_fedavg_f64", X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s), float(f.div),
                  out.data_ptr(), st)
    return out


def _cast_scalars(values: Sequence, dt: np.dtype) -> np.ndarray:
    """The scalars as numpy converts them to the dtype of the operation they enter."""
    if dt.kind == "i":
        return np.array([int(v) for v in values], dtype=dt)
    return round_scalars(values, dt)


def _fold_general(segs: List[torch.Tensor], plan: FoldPlan, weights: Sequence, scores: Optional[Sequence],
                  total, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """numpy's fold where it types the terms one by one (plan.uniform is None:
    strong and weak scalars mixed, numpy-scalar scores, integer rows under
    scores, rows of several dtypes, a strong total), bit for bit, from the
    kernels the uniform folds use.  segs: the rows in order, as [k, P]
    matrices of one dtype each.  Over each run of rows that share a plan entry:
      product   in prod[i]: the rows widened once (exact; an integer to float64
                rounds as numpy's cast does).  Where it is narrower than what
                follows it is formed alone -- one unfinalised one-row launch of
                fa_fold_f16 / fa_fold_f32 per row, a wrapping torch integer
                multiply for integer rows -- and widened exactly
      score     likewise in term[i]
      sum       in acc[i]: fa_fold_f16 / fa_fold_f32 continue the accumulator
                (widened exactly where the dtype grows) over the run, with the
                factors that are still to be applied, or factor 1 over finished
                terms (x * 1 is exact).  An integer sum wraps, so its order is
                free: a torch integer sum.  float64 needs no accumulate step here
                (fa_fold_f64 serves the ingest pipe): nothing is wider, so
                from the first float64 sum on, the widened
                accumulator and every later term are rows of one matrix that
                fa_fedavg_f64 folds once, in order, with the true divisor
      quotient  in plan.quot, by the total rounded to it.
    A few launches per run of rows: this serves odd inputs, not a hot path."""
    if torch.cuda.is_current_stream_capturing():
        raise InvalidParameterShapeError("a fold that numpy types term by term (mixed scalar kinds or row dtypes) "
                                         "does not run under stream capture")
    dts = {*plan.prod, *plan.term, *plan.acc, plan.quot}
    if not dts <= set(_NP_TO_TORCH) or any(x.dtype not in _TORCH_TO_NP for x in segs):
        raise InvalidParameterShapeError(f"unsupported dtype mix: rows {sorted({str(x.dtype) for x in segs})}, "
                                         f"terms and sums {sorted(map(str, dts))}")
    dev, P, Q = segs[0].device, segs[0].shape[1], plan.quot
    st = stream_ptr(dev)
    total = sum(weights) if total is None else total
    div = Q.type(total)
    res = torch.empty(P, dtype=_NP_TO_TORCH[Q], device=dev)
    if out is not None:
        _check_out("out", out, res.dtype, P)
    L = _lib.load()
    ones = lambda k, dt: np.ones(k, dt)

    def factors(dt, a, s):
        if dt == _F16:  # the half factors end on a 4-byte word inside the staged block
            pad = np.zeros(2 + (len(a) & 1), np.float16)
            a, s = np.concatenate([a, pad]), (None if s is None else np.concatenate([s, pad]))
        staged = stage_factors([a] if s is None else [a, s], dev)
        return staged[0], (staged[1] if s is not None else None)

    def pitch(Y):
        return Y.stride(0) if Y.shape[0] > 1 else max(P, 1)

    def fold(Y, dt, a, s, acc):  # acc (+)= the terms fl(fl(Y_r * a_r) * s_r) in row order, all in dt (16/32 bit)
        dst = acc if acc is not None else torch.empty(P, dtype=Y.dtype, device=dev)
        ad, sd = factors(dt, a, s)
        if dt == _F16:
            _lib.check(L.fa_fold_f16(Y.data_ptr(), Y.shape[0], P, pitch(Y), ad.data_ptr(), _ptr(sd), _ptr(acc), 0, 0,
                                     dst.data_ptr(), st), "fa_fold_f16")
        else:
            _lib.check(L.fa_fold_f32(Y.data_ptr(), Y.shape[0], P, pitch(Y), ad.data_ptr(), _ptr(sd), _ptr(acc), 0.0, 0,
                                     dst.data_ptr(), st), "fa_fold_f32")
        return dst

    def products(Y, dt, a):  # [k, P]: fl(Y_r * a_r) in dt, every row on its own
        if dt.kind == "i":
            return Y * torch.from_numpy(a).to(dev)[:, None]  # wraps as numpy's integer multiply
        k, esz = Y.shape[0], dt.itemsize
        T = torch.empty((k, P), dtype=Y.dtype, device=dev)
        ad, _ = factors(dt, a, None)
        for r in range(k):
            x, d, f = Y.data_ptr() + r * Y.stride(0) * esz, T.data_ptr() + r * P * esz, ad.data_ptr() + r * esz
            if dt == _F64:
                _lib.check(L.fa_fedavg_f64(x, 1, P, max(P, 1), f, None, 1.0, d, st), "fa_fedavg_f64")
            elif dt == _F32:
                _lib.check(L.fa_fold_f32(x, 1, P, max(P, 1), f, None, None, 0.0, 0, d, st), "fa_fold_f32")
            else:
                _lib.check(L.fa_fold_f16(x, 1, P, max(P, 1), f, None, None, 0, 0, d, st), "fa_fold_f16")
        return T

    if P == 0:
        return res if out is None else out
    acc, acc_dt = None, None
    tail: list = []  # from the first float64 sum on: (rows [k, P] float64, a, s or None)
    i = 0
    for X in segs:
        r0 = 0
        while r0 < X.shape[0]:
            sig = (plan.prod[i], plan.term[i], plan.acc[i])
            r1 = r0 + 1
            while r1 < X.shape[0] and (plan.prod[i + r1 - r0], plan.term[i + r1 - r0], plan.acc[i + r1 - r0]) == sig:
                r1 += 1
            k = r1 - r0
            d1, d2, D = sig
            w = weights[i:i + k]
            sc = None if scores is None else scores[i:i + k]
            if acc is not None and acc_dt != D:
                if D == _F64:
                    tail.append((acc.to(torch.float64)[None, :], ones(1, _F64), None))
                    acc = None
                else:
                    acc = acc.to(_NP_TO_TORCH[D])
            acc_dt = D
            Y = X[r0:r1].to(_NP_TO_TORCH[d1])
            if d1 == d2 == D:
                a, s = _cast_scalars(w, D), (None if sc is None else _cast_scalars(sc, D))
            else:
                Y = products(Y, d1, _cast_scalars(w, d1))
                if d2 == D:  # the score multiply belongs to the sum's dtype
                    a = ones(k, D) if sc is None else _cast_scalars(sc, D)
                else:  # the finished term is narrower than the running sum
                    if sc is not None:
                        Y = products(Y.to(_NP_TO_TORCH[d2]), d2, _cast_scalars(sc, d2))
                    a = ones(k, D)
                Y, s = Y.to(_NP_TO_TORCH[D]), None
            if D == _F64:
                tail.append((Y, a, s))
            elif D.kind == "i":
                t = Y * torch.from_numpy(a).to(dev)[:, None]
                if s is not None:
                    t = t * torch.from_numpy(s).to(dev)[:, None]
                t = t.sum(0, dtype=Y.dtype)  # a sum that wraps has no order
                acc = t if acc is None else acc + t
            else:
                acc = fold(Y, D, a, s, acc)
            i += k
            r0 = r1
    if tail:
        Y = tail[0][0] if len(tail) == 1 else torch.cat([t[0] for t in tail])
        a = np.concatenate([t[1] for t in tail])
        s = None
        if any(t[2] is not None for t in tail):
            s = np.concatenate([t[2] if t[2] is not None else ones(len(t[1]), _F64) for t in tail])
        ad, sd = factors(_F64, a, s)
        _lib.check(L.fa_fedavg_f64(Y.data_ptr(), Y.shape[0], P, pitch(Y), ad.data_ptr(), _ptr(sd), float(div),
                                   res.data_ptr(), st), "fa_fedavg_f64")
    else:
        acc = acc.to(res.dtype)
        if Q == _F16:
            _lib.check(L.fa_fold_f16(None, 0, P, P, None, None, acc.data_ptr(), int(div.view(np.uint16)), 1,
                                     res.data_ptr(), st), "fa_fold_f16(finalize)")
        elif Q == _F32:
            _lib.check(L.fa_fold_f32(None, 0, P, P, None, None, acc.data_ptr(), float(div), 1, res.data_ptr(), st),
                       "fa_fold_f32(finalize)")
        else:
            ad, _ = factors(_F64, ones(1, _F64), None)
            _lib.check(L.fa_fedavg_f64(acc.data_ptr(), 1, P, P, ad.data_ptr(), None, float(div), res.data_ptr(), st),
                       "fa_fedavg_f64(finalize)")
    if out is not None:
        out.reshape(-1)[:P].copy_(res)
        return out
    return res


_rounds_states: dict = {}
_rounds_lock = threading.Lock()


def rounds_state(device: torch.device, stream: Optional[int] = None) -> ctypes.c_void_p:
    """The library's one-launch-per-step state (fa_rounds) for the launches
    issued on one stream of a device (default: its current stream), kept for
    the life of the process (torch's streams come from fixed pools, so the
    handles a process sees are few).  Launches with one state must not
    overlap: the library orders each launch after the previous launch of its
    state (an event), so even a stream handle reused after its stream was
    destroyed cannot run two launches of one state at once."""
    dev = torch.device(device)
    key = (dev, stream if stream is not None else stream_ptr(dev))
    with _rounds_lock:
        h = _rounds_states.get(key)
        if h is None:
            h = ctypes.c_void_p()
            _lib.call("fa_rounds_create", ctypes.byref(h), dev.index if dev.index is not None else 0)
            _rounds_states[key] = h
        return h


def f32_factors(weights: Sequence, scores: Optional[Sequence] = None, total=None) -> Optional[Factors]:
    """The float32 factors of a fold over float32 (or bf16) rows, or None when
    numpy would promote the result (numpy-scalar weights, scores or total):
    the weak-scalar fast path first, the type scan only when it declines."""
    f = Factors.weak_f32(weights, scores, total)
    if f is not None:
        return f
    if result_dtype(np.dtype(np.float32), list(weights), scores, total) != np.float32:
        return None
    return Factors(weights, scores, np.dtype(np.float32), total=total)


def f16_factors(weights: Sequence, scores: Optional[Sequence] = None, total=None) -> Optional[Factors]:
    """The binary16 factors of a fold over float16 rows that stays float16, or
    None when numpy would promote the result (numpy-scalar weights, scores or
    total of a wider type)."""
    if result_dtype(_F16, list(weights), scores, total) != _F16:
        return None
    with np.errstate(over="ignore"):  # a factor beyond binary16 stays inf, as in the reference
        return Factors(weights, scores, _F16, total=total)


def f64_factors(weights: Sequence, scores: Optional[Sequence] = None, total=None) -> Optional[Factors]:
    """The float64 factors of a fold over float64 rows that stays float64, or
    None when numpy would give another result dtype (weights, scores or total
    of a wider or foreign scalar type: np.longdouble where it is wider than
    double, complex).  Python numbers, np.float64, np.float32 and numpy
    integers all keep it float64."""
    if result_dtype(_F64, list(weights), scores, total) != _F64:
        return None
    return Factors(weights, scores, _F64, total=total)


def int_row_factors(dt, weights: Sequence, scores: Optional[Sequence] = None, total=None):
    """(a int64, s float64 or None, divisor float64) of a fold over rows of
    the integer dtype dt (int32 or int64) that the integer row-table kernels
    compute (fa_fedavg_i32/i64_ptrs, _layers), or None for any other fold.
    fold_plan is asked, so numpy's OverflowError (a Python int the dtype cannot
    hold) is raised here, before any launch.  Taken: every product `layer * n`
    stays dt, and either there are no scores and the whole fold is uniform in
    dt (the quotient float64), or every term, every running sum and the
    quotient are float64 (`* s` of an integer product is float64 under Python
    floats, np.float32 and np.float64 alike).  Not taken: float weights (the
    product is float64), int32 rows under np.int64 weights (the product is
    int64)."""
    dt = np.dtype(dt)
    if dt != np.int32 and dt != np.int64:
        return None
    n = min(len(weights), len(scores) if scores is not None else len(weights))
    if n == 0:
        return None
    plan = fold_plan(dt, weights, scores, total)
    if plan.prod.count(dt) != n:
        return None
    if scores is None:
        if plan.uniform != dt:
            return None
    elif plan.term.count(_F64) != n or plan.acc.count(_F64) != n or plan.quot != _F64:
        return None
    total = sum(weights) if total is None else total
    a = np.array([int(w) for w in weights[:n]], dtype=np.int64)
    s = None if scores is None else round_scalars(list(scores[:n]), _F64)
    return a, s, np.float64(total)


def _int_factors(dt, weights, scores, total) -> Optional[Factors]:
    """int_row_factors as a Factors (its staging), or None."""
    t = int_row_factors(dt, weights, scores, total)
    if t is None:
        return None
    f = Factors.__new__(Factors)
    f.total = sum(weights) if total is None else total
    f.a, f.s, f.div = t
    return f


def _half_bits(div) -> int:
    """The bit pattern of a binary16 divisor (Factors.div of a float16 fold)."""
    return int(np.asarray(div, dtype=np.float16).view(np.uint16))


class StagedFactors:
    """Factors uploaded ONCE (one H2D on the current stream) for the several
    folds of one exchange step (fold_staged): the per-round launches of
    ShardedAggregator read them instead of staging their own per launch.
    dtype: float32 (fp32 / bf16 rows), float16 (the binary16 factors of a
    float16 fold, whose divisor travels as its bit pattern) or float64 (a
    float64 fold's, the divisor a Python float)."""

    def __init__(self, f: Factors, device):
        self.a, self.s = f.to(torch.device(device))
        self.dtype = np.dtype(f.a.dtype)
        self.div = _half_bits(f.div) if self.dtype == _F16 else float(f.div)
        self.n = len(f.a)


def fold_staged(X: torch.Tensor, sf: StagedFactors, *, out: Optional[torch.Tensor] = None,
                out_bf16: Optional[torch.Tensor] = None):
    """fold_stacked with staged factors: fp32 rows into out; bf16 rows into
    out and/or out_bf16 (ABI 5); float16 rows (binary16 factors) into a
    float16 out; float64 rows (float64 factors) into a float64 out, with
    fa_fedavg_f64, the kernel fold_stacked runs.  Returns out or out_bf16 when
    it is the only output, else (out, out_bf16)."""
    N, P, ldx = _check_matrix(X)
    if N != sf.n:
        raise InvalidParameterShapeError(f"{N} rows but {sf.n} staged factors")
    st = stream_ptr(X.device)
    if (X.dtype == torch.float16) != (sf.dtype == _F16) or (X.dtype == torch.float64) != (sf.dtype == _F64):
        raise InvalidParameterShapeError(f"{X.dtype} rows with staged {sf.dtype} factors")
    if X.dtype == torch.float64:
        if torch.cuda.is_current_stream_capturing():
            raise InvalidParameterShapeError("the float64 fold does not run under stream capture")
        if out_bf16 is not None:
            raise InvalidParameterShapeError("out_bf16 is for bfloat16 rows")
        if out is None or not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
                               and out.numel() >= P):
            raise ValueError(f"out must be a contiguous CUDA float64 tensor of >= {P} elements")
        _lib.call("fa_fedavg_f64", X.data_ptr(), N, P, ldx, sf.a.data_ptr(), _ptr(sf.s), sf.div, out.data_ptr(), st)
        return out
    if X.dtype == torch.float16:
        if torch.cuda.is_current_stream_capturing():
            raise InvalidParameterShapeError("the float16 fold does not run under stream capture")
        if out_bf16 is not None:
            raise InvalidParameterShapeError("out_bf16 is for bfloat16 rows")
        if out is None or not (out.is_cuda and out.dtype == torch.float16 and out.is_contiguous()
                               and out.numel() >= P):
            raise ValueError(f"out must be a contiguous CUDA float16 tensor of >= {P} elements")
        _lib.call("fa_fedavg_f16", X.data_ptr(), N, P, ldx, sf.a.data_ptr(), _ptr(sf.s), sf.div, out.data_ptr(), st)
        return out
    for name, t, dt in (("out", out, torch.float32), ("out_bf16", out_bf16, torch.bfloat16)):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= P):
            raise ValueError(f"{name} must be a contiguous CUDA {dt} tensor of >= {P} elements")
    if X.dtype == torch.bfloat16:
        if out is None and out_bf16 is None:
            raise ValueError("fold_staged: bf16 rows need out or out_bf16")
        _lib.call("fa_fedavg_bf16", X.data_ptr(), N, P, ldx, sf.a.data_ptr(), _ptr(sf.s), sf.div, _ptr(out),
                  _ptr(out_bf16), st)
        return out_bf16 if out is None else (out if out_bf16 is None else (out, out_bf16))
    if X.dtype != torch.float32 or out is None or out_bf16 is not None:
        raise ValueError("fold_staged: fp32 rows fold into out (float32), no out_bf16")
    _lib.call("fa_fedavg_f32", X.data_ptr(), N, P, ldx, sf.a.data_ptr(), _ptr(sf.s), sf.div, out.data_ptr(), st)
    return out


def fold_rounds(X: torch.Tensor, weights: Sequence, scores: Optional[Sequence], offsets: Sequence[int], *,
                out=None, out_bf16=None, total=None, state: Optional[ctypes.c_void_p] = None,
                capacity: Optional[int] = None, factors: Optional[Factors] = None,
                out_offsets: Optional[Sequence[int]] = None) -> ctypes.c_void_p:
    """Every exchange round of a step in ONE launch (fa_fedavg_*_rounds): round
    k folds the columns [offsets[k], offsets[k+1]) of X (fp32 or bf16 rows)
    into the same columns of out (fp32) and, for bf16 X, of out_bf16 (the RNE
    copy), on the current stream.  fp32 X needs out; bf16 X needs out,
    out_bf16 or both (ABI 5: a step that exchanges the bf16 copy stores no
    fp32 result); float16 X (factors that keep it float16, f16_factors) needs
    a float16 out and takes no out_bf16 (fa_fedavg_f16_rounds: binary16
    products, sums and quotient, the bits of fold_stacked on each round; not
    with a peer exchange's state); float64 X (factors that keep it float64,
    f64_factors) likewise needs a float64 out (fa_fedavg_f64_rounds: the
    bits of fa_fedavg_f64 on each round).  Returns the rounds state for
    `wait_round` (the current stream's, or `state`: a peer exchange's, fa_peers_rounds): the exchange of
    round k may start, on another stream, as soon as round k is complete,
    while the launch goes on.  Same bits as fold_stacked on each round's
    columns.  out / out_bf16: tensors (at least offsets[-1] elements) or raw
    device addresses (a peer exchange's send buffer), which need `capacity`,
    the elements the address holds.  factors: f32_factors(weights, scores,
    total) when the caller has them already (one step, one rounding).
    out_offsets: round k's results go to output columns [out_offsets[k],
    out_offsets[k] + width k) instead (a rank's slots straight into its chunk
    of the gathered model: the all-gather then runs in place)."""
    N, W, ldx = _check_matrix(X)
    if len(weights) != N or (scores is not None and len(scores) != N):
        raise InvalidParameterShapeError(f"{N} rows but {len(weights)} weights")
    f16, f64 = X.dtype == torch.float16, X.dtype == torch.float64
    if (f16 or f64) and out_bf16 is not None:
        raise InvalidParameterShapeError("out_bf16 is for bfloat16 rows")
    rounds = len(offsets) - 1
    if out_offsets is not None:
        if len(out_offsets) < rounds:
            raise ValueError(f"{len(out_offsets)} output offsets for {rounds} rounds")
        end = max((int(out_offsets[k]) + int(offsets[k + 1]) - int(offsets[k]) for k in range(rounds)), default=0)
    else:
        end = int(offsets[-1]) if len(offsets) else 0
    for name, t, dt in (("out", out, X.dtype if f16 or f64 else torch.float32),
                        ("out_bf16", out_bf16, torch.bfloat16)):
        if t is None:
            continue
        if isinstance(t, int):
            if capacity is None or end > capacity:
                raise ValueError(f"{name}: a raw address needs capacity >= {end} elements (got {capacity})")
        elif not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= end):
            raise ValueError(f"{name} must be a contiguous CUDA {dt} tensor of >= {end} elements")
    if out is None and (X.dtype != torch.bfloat16 or out_bf16 is None):
        raise ValueError("fold_rounds needs out (fp32 rows) or out / out_bf16 (bf16 rows)")
    dev = X.device
    f = factors if factors is not None else (f16_factors if f16 else f64_factors if f64 else f32_factors)(
        weights, scores, total)
    if f is None:
        raise InvalidParameterShapeError("the rounds fold takes factors that keep the rows' arithmetic "
                                         "(Python-number weights)")
    if (np.dtype(f.a.dtype) == _F16) != f16 or (np.dtype(f.a.dtype) == _F64) != f64:
        raise InvalidParameterShapeError(f"{X.dtype} rows with {f.a.dtype} factors")
    offs = (ctypes.c_int64 * len(offsets))(*[int(o) for o in offsets])
    oo = None if out_offsets is None else (ctypes.c_int64 * rounds)(*[int(o) for o in out_offsets[:rounds]])
    st = stream_ptr(dev)
    r = state if state is not None else rounds_state(dev, st)
    addr = (lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr()))
    # the factors from host memory: the library stages them (one C call, _hostf)
    if X.dtype == torch.bfloat16:
        _lib.call("fa_fedavg_bf16_rounds_hostf", r, X.data_ptr(), N, ldx, *f.host(), float(f.div),
                  addr(out), addr(out_bf16), rounds, offs, oo, st)
    elif X.dtype == torch.float32:
        _lib.call("fa_fedavg_f32_rounds_hostf", r, X.data_ptr(), N, ldx, *f.host(), float(f.div),
                  addr(out), rounds, offs, oo, st)
    elif f16:
        # binary16 factors: staged here, once for the step's launch (Factors.to)
        a, s = f.to(dev)
        _lib.call("fa_fedavg_f16_rounds", r, X.data_ptr(), N, ldx, a.data_ptr(), _ptr(s), _half_bits(f.div),
                  addr(out), rounds, offs, oo, st)
    elif f64:
        # float64 factors: staged here, once for the step's launch (Factors.to)
        a, s = f.to(dev)
        _lib.call("fa_fedavg_f64_rounds", r, X.data_ptr(), N, ldx, a.data_ptr(), _ptr(s), float(f.div),
                  addr(out), rounds, offs, oo, st)
    else:
        raise InvalidParameterShapeError(
            f"the rounds fold takes float32, bfloat16, float16 or float64 rows, got {X.dtype}")
    return r


def wait_round(state: ctypes.c_void_p, k: int, stream: torch.cuda.Stream) -> None:
    """Enqueue on `stream` a wait for round k of the last fold_rounds launch."""
    _lib.call("fa_rounds_wait", state, int(k), stream.cuda_stream)


def _equal_stride_view(rows, host_ptrs: np.ndarray, P: int) -> Optional[torch.Tensor]:
    """[N, P] view when the rows sit in ONE storage at a constant forward pitch
    (a whole number of elements of the rows' dtype).

    A device-resident simulation usually hands over `X[i]` rows of one stacked
    tensor (or equal-size slices of one buffer): then the stacked fold reads
    them with ldx = pitch, with no pointer table to build and upload and with
    the narrow-model (LDS-staged) kernels the pointer-list fold lacks.

    Only the first and the last row are asked for their storage: when both lie
    in one storage, every row between them at the constant pitch lies in that
    storage's contiguous range too, so the view reads exactly the bytes the
    rows' own pointers name (as_strided re-checks the bounds)."""
    N = len(rows)
    if N < 2 or P == 0:
        return None
    esize = rows[0].element_size()
    step = int(host_ptrs[1] - host_ptrs[0])
    if step < P * esize or step % esize:
        return None
    if (np.diff(host_ptrs) != step).any():
        return None
    base, last = rows[0], rows[-1]
    if last.untyped_storage().data_ptr() != base.untyped_storage().data_ptr():
        return None
    return base.as_strided((N, P), (step // esize, 1))


_dtype_of = operator.attrgetter("dtype")
# dtypes the library folds through a device table of row pointers
_ROW_TABLE_DTYPES = (torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int32, torch.int64,
                     *_FP8_FORMATS)
_INT_ROWS = {torch.int32: "fa_fedavg_i32_ptrs", torch.int64: "fa_fedavg_i64_ptrs"}
# dtypes whose row-table fold does not run under a stream capture: they keep the route they had before it
_NO_CAPTURE_TABLE = (torch.float64, torch.int32, torch.int64)
# process-wide route counters (diagnostics, as StreamingFold.stats): 16-bit and
# float64 folds that ran through a row table (layers: a one-launch model fold
# counts each of its layers), layer groups copied into a stacked matrix,
# one-launch model folds (fa_fedavg_*_layers), integer folds that ran through a
# row table (counted as the float64 ones), promoted stacked folds that read
# the narrow rows (fa_fedavg_widen; nothing else counts there), layers folded
# through a widening row table (fa_fedavg_widen_ptrs, or each layer of a
# fa_fedavg_widen_layers launch) and those launches (they move no other counter),
# fp8 folds (fa_fedavg_fp8 and fa_fedavg_fp8_ptrs: one per layer of a model),
# MX folds (fa_fedavg_mx and fa_fedavg_mx_ptrs, likewise; an MX layer-table
# launch, fa_fedavg_mx_layers / _mx_q_layers, counts each of its non-empty layers
# there and itself in mx_table_folds)
stats = {"rows16_folds": 0, "rows64_folds": 0, "stacked_groups": 0, "layer_table_folds": 0, "rows_int_folds": 0,
         "widened_folds": 0, "widened_row_folds": 0, "widened_table_folds": 0, "fp8_folds": 0,
         "mx_folds": 0, "mx_out_folds": 0, "mx_table_folds": 0, "nvfp4_folds": 0}


class RowSet:
    """N client rows already on the GPU, prepared once for repeated folds.

    A device-resident simulation keeps each client's update in its own
    persistent tensor and refolds the same rows every round.  Building a
    RowSet validates the rows and looks at their placement ONCE:
      - rows of one allocation at a constant forward pitch (X[i] of a stacked
        tensor) become one [N, P] strided view: the stacked fold, no table;
      - other fp32 rows get a device table of row pointers for
        fa_fedavg_f32_ptrs_aligned (every row 16-B aligned) or
        fa_fedavg_f32_ptrs (any alignment);
      - other bfloat16 / float16 / float64 / fp8 rows get the same table for
        fa_fedavg_bf16_ptrs / fa_fedavg_f16_ptrs / fa_fedavg_f64_ptrs /
        fa_fedavg_fp8_ptrs (`aligned` picks the kernels);
      - other int32 / int64 rows get the same table for fa_fedavg_i32_ptrs /
        fa_fedavg_i64_ptrs, which fold_rows takes where int_row_factors
        accepts the fold.
    fold_rows(rowset, weights) then costs the factor upload and the kernel.
    The RowSet keeps the tensors alive; their CONTENTS may change between
    folds, their storage may not (re-create the RowSet after reallocating).

    block_scales: the rows are MX rows (fp8, or float4_e2m1fn_x2 with two
    columns per byte) and block_scales[i] holds row i's ceil(columns / 32) E8M0
    bytes, separately allocated, at any alignment: one device table of the 2N
    bases for fa_fedavg_mx_ptrs (`cols`: the columns of the fold)."""

    scale_rows = None  # the E8M0 scale rows of an MX row set (a set assembled without __init__ has none)
    block = 32  # the elements per scale byte: 32 (MX) or 16 (NVFP4: float8_e4m3fn scale rows)

    def __init__(self, rows: Sequence[torch.Tensor], block_scales: Optional[Sequence[torch.Tensor]] = None):
        rows = list(rows)
        N = len(rows)
        if N == 0:
            _lib.check(_lib.FA_ERR_NO_CLIENTS, "RowSet")
        r0 = rows[0]
        P, dev, dt = r0.numel(), r0.device, r0.dtype
        if not r0.is_cuda:
            raise ValueError("rows must be CUDA (HIP) tensors")
        # one C-level pass per property (a Python loop over 1024 rows with a
        # reshape per row cost ~1 ms per call, more than the fold of 1024 x 67K)
        if (set(map(torch.Tensor.numel, rows)) != {P} or set(map(_dtype_of, rows)) != {dt}
                or not all(map(torch.Tensor.is_contiguous, rows))
                or set(map(torch.Tensor.get_device, rows)) != {r0.get_device()}):
            raise InvalidParameterShapeError("all rows must be contiguous with equal size, dtype, device")
        self.rows = rows
        self.N, self.P, self.device, self.dtype = N, P, dev, dt
        self.view = None
        self.ptrs = None
        self.host_ptrs = None
        self.aligned = False
        if block_scales is not None:
            self._mx_table(list(block_scales))
            return
        # (float64 and integer rows met under a stream capture keep the stacked copy they had before the row table)
        if dt in _ROW_TABLE_DTYPES and P > 0 and not (dt in _NO_CAPTURE_TABLE
                                                      and torch.cuda.is_current_stream_capturing()):
            host_ptrs = self.host_ptrs = np.fromiter(map(torch.Tensor.data_ptr, rows), dtype=np.int64, count=N)
            self.view = _equal_stride_view(rows, host_ptrs, P)
            if self.view is None:
                self.ptrs = torch.from_numpy(host_ptrs).to(dev)
                self.aligned = not (host_ptrs % 16).any()

    def _mx_table(self, es: list) -> None:
        """The table of an MX row set: N data bases, then the N scale-row bases."""
        N, dev = self.N, self.device
        if self.dtype not in _MX_FORMATS:
            raise InvalidParameterShapeError(f"block_scales are for fp8 / float4_e2m1fn_x2 rows, got {self.dtype}")
        self.cols = _mx_cols(self.dtype, self.P)
        if len(es) != N:
            raise InvalidParameterShapeError(f"{N} rows but {len(es)} block-scale rows")
        for i, e in enumerate(es):
            blk = _block_scale_kind(self.dtype, e, f"block_scales[{i}]")
            if i == 0:
                self.block = blk  # 32: MX rows; 16: NVFP4 rows
            elif blk != self.block:
                raise InvalidParameterShapeError(f"block_scales[{i}]: the rows of one set fold in one format, MXFP4 (E8M0 "
                                                 f"scales) or NVFP4 (float8_e4m3fn scales), got {e.dtype}")
            nb = (self.cols + blk - 1) // blk
            if e.numel() != nb or not e.is_contiguous() or e.device != dev:
                raise InvalidParameterShapeError(f"block_scales[{i}]: {e.numel()} scale bytes for {self.cols} columns "
                                                 f"(one per {blk}: {nb}, contiguous, on {dev})")
        self.scale_rows = es
        if self.P > 0:
            self.host_ptrs = np.fromiter(map(torch.Tensor.data_ptr, self.rows + es), dtype=np.int64, count=2 * N)
            self.ptrs = torch.from_numpy(self.host_ptrs).to(dev)
            self.aligned = not (self.host_ptrs[:N] % 16).any()
            if self.block == _lib.FA_NVFP4_BLOCK:  # the vector path reads a unit's two scale bytes in one 16-bit load
                self.aligned = self.aligned and not (self.host_ptrs[N:] % 2).any()

    def overlaps(self, t: torch.Tensor) -> bool:
        """Does tensor t share a byte with any row (or scale row)?"""
        if self.host_ptrs is None or self.P == 0 or t.numel() == 0:
            return False
        lo = t.data_ptr()
        hi = lo + t.numel() * t.element_size()
        size = self.P * self.rows[0].element_size()
        if self.scale_rows is not None:
            size = np.repeat([size, self.scale_rows[0].numel()], self.N)
        return bool(np.any((self.host_ptrs < hi) & (lo < self.host_ptrs + size)))

    def stacked(self) -> torch.Tensor:
        """The rows copied into one [N, P] tensor (the fallbacks without a row-table fold)."""
        return torch.stack([r.reshape(-1) for r in self.rows])


def _check_out(name: str, t: Optional[torch.Tensor], dt: torch.dtype, P: int) -> None:
    if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= P):
        raise ValueError(f"{name} must be a contiguous CUDA {dt} tensor of >= {P} elements")


def _fold_rows_bf16(rs: "RowSet", weights, scores, out, total, want_bf16, out_bf16):
    """bf16 rows through the row table (fa_fedavg_bf16_ptrs): the outputs and
    the factors of fold_stacked's bf16 branch, no stacking copy."""
    dev, P = rs.device, rs.P
    _check_out("out", out, torch.float32, P)
    _check_out("out_bf16", out_bf16, torch.bfloat16, P)
    f = Factors.weak_f32(weights, scores, total) or Factors(weights, scores, np.dtype(np.float32), total=total)
    # an output over a client row: the table lives in device memory, the library
    # cannot see the alias.  Fold into a fresh buffer, then copy.
    dst, dstb = out, out_bf16
    if out is not None and rs.overlaps(out):
        out = None
    outb = None if (out_bf16 is not None and rs.overlaps(out_bf16)) else out_bf16
    if outb is None and (want_bf16 or out_bf16 is not None):
        outb = torch.empty(P, dtype=torch.bfloat16, device=dev)
    if out is None and (dst is not None or outb is None or want_bf16):
        out = torch.empty(P, dtype=torch.float32, device=dev)
    aligned = rs.aligned and (out is None or out.data_ptr() % 16 == 0) and (outb is None or outb.data_ptr() % 16 == 0)
    st = stream_ptr(dev)
    if torch.cuda.is_current_stream_capturing():
        a, s = _captured_factors(f, dev)
        _lib.call("fa_fedavg_bf16_ptrs", rs.ptrs.data_ptr(), rs.N, P, a.data_ptr(), _ptr(s), float(f.div),
                  int(aligned), _ptr(out), _ptr(outb), st)
    else:
        _lib.call("fa_fedavg_bf16_ptrs_hostf", rs.ptrs.data_ptr(), rs.N, P, *f.host(), float(f.div),
                  int(aligned), _ptr(out), _ptr(outb), st)
    stats["rows16_folds"] += 1
    if dst is not None and dst is not out:
        dst.reshape(-1)[:P].copy_(out)
        out = dst
    if dstb is not None and dstb is not outb:
        dstb.reshape(-1)[:P].copy_(outb)
        outb = dstb
    if want_bf16:
        return out, outb
    if out_bf16 is not None:
        return outb if out is None else (out, outb)
    return out


class _MXOut:
    """The buffers of a fold's MX result (out_format= / out_mx= of fold_stacked
    and fold_rows): the caller's, or fresh ones where it gave none or gave
    buffers that share bytes with an input (clash), copied back by result()."""

    def __init__(self, out_format, out_mx, P: int, dev, bf16: bool, clash):
        if out_format is None:
            out_format = out_mx[0].dtype
        if out_format not in _MX_FORMATS:
            raise InvalidParameterShapeError("out_format must be float8_e4m3fn, float8_e5m2 or float4_e2m1fn_x2, got "
                                             f"{out_format}")
        if bf16:
            raise InvalidParameterShapeError("out_format gives an MX result: want_bf16 / out_bf16 do not go with it")
        fp4 = out_format == torch.float4_e2m1fn_x2
        if fp4 and P % 2:
            raise InvalidParameterShapeError(f"a float4_e2m1fn_x2 result holds two columns per byte: {P} columns")
        nq, nb = (P // 2 if fp4 else P), (P + 31) // 32
        self.fmt, self.dst = _MX_FORMATS[out_format], out_mx
        if out_mx is not None:
            q, e = out_mx
            if not (isinstance(q, torch.Tensor) and q.dtype == out_format and q.device == dev and q.is_contiguous()
                    and q.numel() == nq):
                raise InvalidParameterShapeError(f"out_mx[0] must be a contiguous {out_format} tensor of {nq} elements "
                                                 f"on {dev}")
            if not (isinstance(e, torch.Tensor) and e.dtype in _MX_SCALE_DTYPES and e.device == dev
                    and e.is_contiguous() and e.numel() == nb):
                raise InvalidParameterShapeError(f"out_mx[1] must hold {nb} contiguous E8M0 bytes (float8_e8m0fnu or "
                                                 f"uint8) on {dev}")
        self.fresh = out_mx is None or clash(out_mx[0]) or clash(out_mx[1])
        if self.fresh:
            self.q = torch.empty(nq, dtype=torch.uint8, device=dev).view(out_format)
            self.e = torch.empty(nb, dtype=torch.uint8, device=dev).view(torch.float8_e8m0fnu)
        else:
            self.q, self.e = out_mx[0].reshape(-1), out_mx[1].reshape(-1)

    def args(self):
        return self.fmt, self.q.data_ptr(), self.e.data_ptr()

    def result(self) -> "MXLayer":
        stats["mx_out_folds"] += 1
        if self.dst is not None and self.fresh:
            self.dst[0].view(torch.uint8).reshape(-1).copy_(self.q.view(torch.uint8))
            self.dst[1].view(torch.uint8).reshape(-1).copy_(self.e.view(torch.uint8))
            return MXLayer(self.dst[0].reshape(-1), self.dst[1].reshape(-1))
        return MXLayer(self.q, self.e)


def _fold_fp8(X: Optional[torch.Tensor], rs: Optional["RowSet"], weights, scores, scales, out, total, want_bf16,
              out_bf16, out_format=None, out_mx=None):
    """fp8 rows, a stacked [N, P] matrix X (fa_fedavg_fp8) or the row table of
    rs (fa_fedavg_fp8_ptrs): float32 factors and scales in ONE staged upload,
    the bf16 fold's outputs.  The outputs are wider than the rows, so one that
    shares bytes with a row is folded into a fresh buffer and copied."""
    if torch.cuda.is_current_stream_capturing():
        raise InvalidParameterShapeError("the fp8 fold does not run under stream capture "
                                         "(its factors and scales are staged by a copy the graph would not own)")
    if X is not None:
        N, P, ldx = _check_matrix(X)
        dev, fmt = X.device, _FP8_FORMATS[X.dtype]
    else:
        N, P, dev, fmt = rs.N, rs.P, rs.device, _FP8_FORMATS[rs.dtype]
    if scales is not None and len(scales) != N:
        raise InvalidParameterShapeError(f"{N} rows but {len(scales)} scales")
    _check_out("out", out, torch.float32, P)
    _check_out("out_bf16", out_bf16, torch.bfloat16, P)

    def clash(t) -> bool:
        if t is None or P == 0:
            return False
        if X is None:
            return rs.overlaps(t)
        lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        return lo < X.data_ptr() + (N - 1) * ldx + P and X.data_ptr() < hi

    qo = None
    if out_format is not None or out_mx is not None:
        qo = _MXOut(out_format, out_mx, P, dev, want_bf16 or out_bf16 is not None, clash)
    dst, dstb = out, out_bf16
    if clash(out):
        out = None
    outb = None if clash(out_bf16) else out_bf16
    if outb is None and (want_bf16 or out_bf16 is not None):
        outb = torch.empty(P, dtype=torch.bfloat16, device=dev)
    if out is None and (dst is not None or (outb is None and qo is None) or want_bf16):
        out = torch.empty(P, dtype=torch.float32, device=dev)
    f = Factors.weak_f32(weights, scores, total) or Factors(weights, scores, _F32, total=total)
    parts = [f.a] if f.s is None else [f.a, f.s]
    if scales is not None:
        c = weak_f32(scales)
        parts.append(c if c is not None else round_scalars(scales, _F32))
    staged = stage_factors(parts, dev)
    a, s = staged[0], (staged[1] if f.s is not None else None)
    c = staged[-1] if scales is not None else None
    if qo is not None and X is not None:
        _lib.call("fa_fedavg_fp8_q", fmt, X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s), _ptr(c), float(f.div),
                  _ptr(out), *qo.args(), stream_ptr(dev))
    elif qo is not None:
        aligned = rs.aligned and (out is None or out.data_ptr() % 16 == 0) and qo.q.data_ptr() % 16 == 0
        _lib.call("fa_fedavg_fp8_q_ptrs", fmt, rs.ptrs.data_ptr(), N, P, a.data_ptr(), _ptr(s), _ptr(c), float(f.div),
                  int(aligned), _ptr(out), *qo.args(), stream_ptr(dev))
    elif X is not None:
        _lib.call("fa_fedavg_fp8", fmt, X.data_ptr(), N, P, ldx, a.data_ptr(), _ptr(s), _ptr(c), float(f.div),
                  _ptr(out), _ptr(outb), stream_ptr(dev))
    else:
        aligned = (rs.aligned and (out is None or out.data_ptr() % 16 == 0)
                   and (outb is None or outb.data_ptr() % 16 == 0))
        _lib.call("fa_fedavg_fp8_ptrs", fmt, rs.ptrs.data_ptr(), N, P, a.data_ptr(), _ptr(s), _ptr(c), float(f.div),
                  int(aligned), _ptr(out), _ptr(outb), stream_ptr(dev))
    stats["fp8_folds"] += 1
    if dst is not None and dst is not out:
        dst.reshape(-1)[:P].copy_(out)
        out = dst
    if dstb is not None and dstb is not outb:
        dstb.reshape(-1)[:P].copy_(outb)
        outb = dstb
    if qo is not None:
        return qo.result()
    if want_bf16:
        return out, outb
    if out_bf16 is not None:
        return outb if out is None else (out, outb)
    return out


def _fold_mx(X: Optional[torch.Tensor], E: Optional[torch.Tensor], rs: Optional["RowSet"], weights, scores, scales,
             out, total, want_bf16, out_bf16, out_format=None, out_mx=None):
    """MX rows, a stacked byte matrix X with its scale bytes E (fa_fedavg_mx) or
    the 2N-pointer table of rs (fa_fedavg_mx_ptrs): float32 factors and scales
    in ONE staged upload, the bf16 fold's outputs.  Everything is decided here
    on the host before the launch; an output that shares bytes with a row or a
    scale row is folded into a fresh buffer and copied."""
    nv = _is_nvfp4(E) if X is not None else rs.block == _lib.FA_NVFP4_BLOCK
    if torch.cuda.is_current_stream_capturing():
        raise InvalidParameterShapeError(f"the {'NVFP4' if nv else 'MX'} fold does not run under stream capture "
                                         "(its factors and scales are staged by a copy the graph would not own)")
    if X is not None:
        N, Pb, ldx = _check_matrix(X)
        if X.dtype not in _MX_FORMATS:
            raise InvalidParameterShapeError(f"block_scales are for fp8 / float4_e2m1fn_x2 rows, got {X.dtype}")
        if E is None:
            raise InvalidParameterShapeError(f"{X.dtype} rows fold only with their block_scales")
        dev, fmt, P = X.device, _MX_FORMATS[X.dtype], _mx_cols(X.dtype, Pb)
        blk = _block_scale_kind(X.dtype, E, "block_scales")
        nb = (P + blk - 1) // blk
        if E.device != dev or tuple(E.shape) != (N, nb) or (nb > 1 and E.stride(1) != 1):
            raise InvalidParameterShapeError(f"block_scales must be [{N}, {nb}] on {dev} with unit column stride (one "
                                             f"byte per {blk} of {P} columns), got {tuple(E.shape)}")
        lde = E.stride(0) if N > 1 else max(nb, 1)
        if lde < nb:
            raise InvalidParameterShapeError(f"block_scales rows overlap (pitch {lde} < {nb})")
        spans = [(X.data_ptr(), (N - 1) * ldx + Pb), (E.data_ptr(), (N - 1) * lde + nb)]
    else:
        N, P, dev, fmt = rs.N, rs.cols, rs.device, _MX_FORMATS[rs.dtype]
    if fmt == _lib.FA_MX_E2M1 and P % 2:
        raise InvalidParameterShapeError(f"float4_e2m1fn_x2 rows hold two columns per byte: {P} columns")
    if scales is not None and len(scales) != N:
        raise InvalidParameterShapeError(f"{N} rows but {len(scales)} scales")
    if nv and (out_format is not None or out_mx is not None):
        raise InvalidParameterShapeError("out_format / out_mx do not go with NVFP4 rows (float8_e4m3fn block scales): "
                                         "their fold returns float32 / bfloat16")
    _check_out("out", out, torch.float32, P)
    _check_out("out_bf16", out_bf16, torch.bfloat16, P)

    def clash(t) -> bool:
        if t is None or P == 0:
            return False
        if X is None:
            return rs.overlaps(t)
        lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        return any(lo < p + n and p < hi for p, n in spans)

    qo = None
    if out_format is not None or out_mx is not None:
        qo = _MXOut(out_format, out_mx, P, dev, want_bf16 or out_bf16 is not None, clash)
    dst, dstb = out, out_bf16
    if clash(out):
        out = None
    outb = None if clash(out_bf16) else out_bf16
    if outb is None and (want_bf16 or out_bf16 is not None):
        outb = torch.empty(P, dtype=torch.bfloat16, device=dev)
    if out is None and (dst is not None or (outb is None and qo is None) or want_bf16):
        out = torch.empty(P, dtype=torch.float32, device=dev)
    f = Factors.weak_f32(weights, scores, total) or Factors(weights, scores, _F32, total=total)
    parts = [f.a] if f.s is None else [f.a, f.s]
    if scales is not None:
        c = weak_f32(scales)
        parts.append(c if c is not None else round_scalars(scales, _F32))
    staged = stage_factors(parts, dev)
    a, s = staged[0], (staged[1] if f.s is not None else None)
    c = staged[-1] if scales is not None else None
    if nv and X is not None:
        _lib.call("fa_fedavg_nvfp4", X.data_ptr(), E.data_ptr(), N, P, ldx, lde, a.data_ptr(), _ptr(s), _ptr(c),
                  float(f.div), _ptr(out), _ptr(outb), stream_ptr(dev))
    elif nv:
        aligned = (rs.aligned and (out is None or out.data_ptr() % 16 == 0)
                   and (outb is None or outb.data_ptr() % 16 == 0))
        xi = rs.ptrs.data_ptr() if P else 0
        _lib.call("fa_fedavg_nvfp4_ptrs", xi, xi + 8 * N, N, P, a.data_ptr(), _ptr(s), _ptr(c), float(f.div),
                  int(aligned), _ptr(out), _ptr(outb), stream_ptr(dev))
    elif qo is not None and X is not None:
        _lib.call("fa_fedavg_mx_q", fmt, X.data_ptr(), E.data_ptr(), N, P, ldx, lde, a.data_ptr(), _ptr(s), _ptr(c),
                  float(f.div), _ptr(out), *qo.args(), stream_ptr(dev))
    elif qo is not None:
        aligned = rs.aligned and (out is None or out.data_ptr() % 16 == 0) and qo.q.data_ptr() % 16 == 0
        xi = rs.ptrs.data_ptr() if P else 0
        _lib.call("fa_fedavg_mx_q_ptrs", fmt, xi, xi + 8 * N, N, P, a.data_ptr(), _ptr(s), _ptr(c), float(f.div),
                  int(aligned), _ptr(out), *qo.args(), stream_ptr(dev))
    elif X is not None:
        _lib.call("fa_fedavg_mx", fmt, X.data_ptr(), E.data_ptr(), N, P, ldx, lde, a.data_ptr(), _ptr(s), _ptr(c),
                  float(f.div), _ptr(out), _ptr(outb), stream_ptr(dev))
    else:
        aligned = (rs.aligned and (out is None or out.data_ptr() % 16 == 0)
                   and (outb is None or outb.data_ptr() % 16 == 0))
        xi = rs.ptrs.data_ptr() if P else 0
        _lib.call("fa_fedavg_mx_ptrs", fmt, xi, xi + 8 * N, N, P, a.data_ptr(), _ptr(s), _ptr(c), float(f.div),
                  int(aligned), _ptr(out), _ptr(outb), stream_ptr(dev))
    stats["nvfp4_folds" if nv else "mx_folds"] += 1
    if dst is not None and dst is not out:
        dst.reshape(-1)[:P].copy_(out)
        out = dst
    if dstb is not None and dstb is not outb:
        dstb.reshape(-1)[:P].copy_(outb)
        outb = dstb
    if qo is not None:
        return qo.result()
    if want_bf16:
        return out, outb
    if out_bf16 is not None:
        return outb if out is None else (out, outb)
    return out


def _fold_rows_f16(rs: "RowSet", weights, scores, out, total):
    """float16 rows whose result stays float16 through the row table
    (fa_fedavg_f16_ptrs): the factors of fold_stacked's float16 branch."""
    dev, P = rs.device, rs.P
    if torch.cuda.is_current_stream_capturing():
        raise InvalidParameterShapeError("the float16 fold does not run under stream capture "
                                         "(the captured factor fill carries float32 factors only)")
    _check_out("out", out, torch.float16, P)
    dst = out
    if out is not None and rs.overlaps(out):
        out = None
    if out is None:
        out = torch.empty(P, dtype=torch.float16, device=dev)
    f = Factors(weights, scores, np.dtype(np.float16), total=total)
    a, s = f.to(dev)
    aligned = rs.aligned and out.data_ptr() % 16 == 0
    _lib.call("fa_fedavg_f16_ptrs", rs.ptrs.data_ptr(), rs.N, P, a.data_ptr(), _ptr(s),
              int(np.asarray(f.div, dtype=np.float16).view(np.uint16)), int(aligned), out.data_ptr(),
              stream_ptr(dev))
    stats["rows16_folds"] += 1
    if dst is not None and dst is not out:
        dst.reshape(-1)[:P].copy_(out)
        return dst
    return out


def _fold_rows_f64(rs: "RowSet", weights, scores, out, total):
    """float64 rows whose result stays float64 through the row table
    (fa_fedavg_f64_ptrs): the factors of fold_stacked's float64 branch."""
    dev, P = rs.device, rs.P
    _check_out("out", out, torch.float64, P)
    dst = out
    if out is not None and rs.overlaps(out):
        out = None
    if out is None:
        out = torch.empty(P, dtype=torch.float64, device=dev)
    f = Factors(weights, scores, _F64, total=total)
    a, s = f.to(dev)
    aligned = rs.aligned and out.data_ptr() % 16 == 0
    _lib.call("fa_fedavg_f64_ptrs", rs.ptrs.data_ptr(), rs.N, P, a.data_ptr(), _ptr(s), float(f.div), int(aligned),
              out.data_ptr(), stream_ptr(dev))
    stats["rows64_folds"] += 1
    if dst is not None and dst is not out:
        dst.reshape(-1)[:P].copy_(out)
        return dst
    return out


def _fold_rows_int(rs: "RowSet", f: Factors, out):
    """int32 / int64 rows through the row table (fa_fedavg_i32_ptrs /
    fa_fedavg_i64_ptrs) with the factors of int_row_factors; float64 out."""
    dev, P = rs.device, rs.P
    _check_out("out", out, torch.float64, P)
    dst = out
    if out is not None and rs.overlaps(out):
        out = None
    if out is None:
        out = torch.empty(P, dtype=torch.float64, device=dev)
    a, s = f.to(dev)
    aligned = rs.aligned and out.data_ptr() % 16 == 0
    _lib.call(_INT_ROWS[rs.dtype], rs.ptrs.data_ptr(), rs.N, P, a.data_ptr(), _ptr(s), float(f.div), int(aligned),
              out.data_ptr(), stream_ptr(dev))
    stats["rows_int_folds"] += 1
    if dst is not None and dst is not out:
        dst.reshape(-1)[:P].copy_(out)
        return dst
    return out


def _fold_rows_widen(rs: "RowSet", kind: int, f: Factors, out):
    """Promoted rows through the row table (fa_fedavg_widen_ptrs) with the
    factors of widen_factors: neither a stacked nor a widened copy; out in the
    promoted dtype."""
    dev, P = rs.device, rs.P
    res_dt = _widen_out_dtype(kind)
    _check_out("out", out, res_dt, P)
    dst = out
    if out is not None and rs.overlaps(out):
        out = None
    if out is None:
        out = torch.empty(P, dtype=res_dt, device=dev)
    a, s = f.to(dev)
    aligned = rs.aligned and out.data_ptr() % 16 == 0
    _lib.call("fa_fedavg_widen_ptrs", kind, rs.ptrs.data_ptr(), rs.N, P, a.data_ptr(), _ptr(s), float(f.div),
              int(aligned), out.data_ptr(), stream_ptr(dev))
    stats["widened_row_folds"] += 1
    if dst is not None and dst is not out:
        dst.reshape(-1)[:P].copy_(out)
        return dst
    return out


def fold_rows(rows, weights: Sequence, scores: Optional[Sequence] = None, *,
              out: Optional[torch.Tensor] = None, total=None, want_bf16: bool = False,
              out_bf16: Optional[torch.Tensor] = None, scales: Optional[Sequence] = None,
              block_scales: Optional[Sequence[torch.Tensor]] = None, out_format: Optional[torch.dtype] = None,
              out_mx=None):
    """The fold over separately allocated 1-D CUDA rows (no stacking copy for
    fp32, bfloat16, float16 / float64 rows whose result stays in their dtype,
    int32 / int64 rows whose products stay in their dtype: int_row_factors, and
    rows numpy promotes as a whole where a widening kernel converts them on
    load: widen_factors).  `rows` is a
    RowSet (prepared once, reusable) or a sequence of tensors (a RowSet is
    built for this call).  want_bf16 / out_bf16: as fold_stacked (bf16 and
    fp8 rows); scales: as fold_stacked (fp8 rows, folded through their own row
    table); block_scales: the rows are MX rows, block_scales[i] row i's E8M0
    bytes (RowSet's block_scales=; a RowSet built with them needs none here);
    out_format / out_mx: as fold_stacked (fp8 and MX rows)."""
    rs = rows if isinstance(rows, RowSet) else RowSet(rows, block_scales)
    if len(weights) != rs.N or (scores is not None and len(scores) != rs.N):
        raise InvalidParameterShapeError(f"{rs.N} rows but {len(weights)} weights"
                                         + ("" if scores is None else f" / {len(scores)} scores"))
    if rs.scale_rows is not None:
        if block_scales is not None and rs is rows:
            raise InvalidParameterShapeError("this RowSet already holds its block_scales")
        return _fold_mx(None, None, rs, weights, scores, scales, out, total, want_bf16, out_bf16, out_format, out_mx)
    if block_scales is not None or rs.dtype == torch.float4_e2m1fn_x2:
        raise InvalidParameterShapeError(f"{rs.dtype} rows and block_scales: build the RowSet with block_scales=")
    if rs.dtype in _FP8_FORMATS:
        if rs.view is not None or rs.P == 0:
            # rows of one allocation at a fixed pitch (or no columns): the stacked fold, no pointer table
            X = rs.view if rs.view is not None else torch.empty((rs.N, 0), dtype=rs.dtype, device=rs.device)
            return _fold_fp8(X, None, weights, scores, scales, out, total, want_bf16, out_bf16, out_format, out_mx)
        return _fold_fp8(None, rs, weights, scores, scales, out, total, want_bf16, out_bf16, out_format, out_mx)
    if out_format is not None or out_mx is not None:
        raise InvalidParameterShapeError(f"out_format / out_mx are for fp8 and MX rows, got {rs.dtype}")
    if scales is not None:
        raise InvalidParameterShapeError(f"scales are for fp8 rows, got {rs.dtype}")
    if out_bf16 is not None and rs.dtype != torch.bfloat16:
        raise InvalidParameterShapeError("out_bf16 is for bfloat16 rows")
    if rs.dtype == torch.bfloat16:
        if rs.view is not None or rs.P == 0:
            # rows of one allocation at a fixed pitch: the stacked fold, no pointer table
            X = rs.view if rs.view is not None else rs.stacked()
            return fold_stacked(X, weights, scores, out=out, total=total, want_bf16=want_bf16, out_bf16=out_bf16)
        return _fold_rows_bf16(rs, weights, scores, out, total, want_bf16, out_bf16)
    if (rs.dtype == torch.float16 and rs.view is None and rs.P > 0
            and result_dtype(np.dtype(np.float16), weights, scores, total) == np.float16):
        return _fold_rows_f16(rs, weights, scores, out, total)
    if (rs.dtype == torch.float64 and rs.view is None and rs.P > 0
            and not torch.cuda.is_current_stream_capturing()  # captured float64 rows keep the stacked route
            and result_dtype(_F64, weights, scores, total) == _F64):
        return _fold_rows_f64(rs, weights, scores, out, total)
    if (rs.dtype in _INT_ROWS and rs.ptrs is not None and rs.P > 0
            and not torch.cuda.is_current_stream_capturing()):  # captured integer rows keep the stacked route
        # integer rows whose every product stays in their dtype (numpy's OverflowError comes from here)
        fi = _int_factors(_TORCH_TO_NP[rs.dtype], weights, scores, total)
        if fi is not None:
            return _fold_rows_int(rs, fi, out)
    fw = Factors.weak_f32(weights, scores, total) if rs.dtype == torch.float32 else None
    if fw is None and (rs.dtype != torch.float32
                       or result_dtype(np.dtype(np.float32), weights, scores, total) != np.float32):
        # numpy promotes the fold (float16 rows under np.float32 weights, float32
        # rows under an np.int64 from len(), integer rows under float weights):
        # rows apart go through the widening row table, converted on load
        if (rs.view is None and rs.ptrs is not None and rs.P > 0 and rs.dtype in _TORCH_TO_NP
                and not torch.cuda.is_current_stream_capturing()):
            wf = widen_factors(_TORCH_TO_NP[rs.dtype], weights, scores, total)
            if wf is not None:
                return _fold_rows_widen(rs, *wf, out)
        # no row-table fold for this dtype / these factors: the stacked fold, over
        # the rows' own storage when they sit at a fixed pitch, else over a stacked copy
        X = rs.view if rs.view is not None else rs.stacked()
        return fold_stacked(X, weights, scores, out=out, total=total)
    if rs.view is not None or rs.P == 0:
        # rows of one allocation at a fixed pitch: the stacked fold, no pointer table
        X = rs.view if rs.view is not None else rs.stacked()
        return fold_stacked(X, weights, scores, out=out, total=total)
    dev = rs.device
    f = fw or Factors(weights, scores, np.dtype(np.float32), total=total)
    dst = out
    if out is not None and rs.overlaps(out):
        # out over a client row: the row table lives in device memory, so the
        # library cannot see the alias, and the tuner's first call of a shape
        # runs several launches into out (a later one would read what an earlier
        # wrote).  Fold into a fresh buffer, then copy.
        out = None
    out = out if out is not None else torch.empty(rs.P, dtype=torch.float32, device=dev)
    aligned = rs.aligned and out.data_ptr() % 16 == 0
    if torch.cuda.is_current_stream_capturing():
        a, s = _captured_factors(f, dev)
        _lib.call("fa_fedavg_f32_ptrs_aligned" if aligned else "fa_fedavg_f32_ptrs", rs.ptrs.data_ptr(), rs.N, rs.P,
                  a.data_ptr(), _ptr(s), float(f.div), out.data_ptr(), stream_ptr(dev))
    else:
        _lib.call("fa_fedavg_f32_ptrs_hostf", rs.ptrs.data_ptr(), rs.N, rs.P, *f.host(), float(f.div),
                  int(aligned), out.data_ptr(), stream_ptr(dev))
    if dst is not None and dst is not out:
        dst.copy_(out)
        return dst
    return out


# ---------------------------------------------------------------------------
# every layer of a device-resident model in one launch (fa_fedavg_*_layers)
# ---------------------------------------------------------------------------
# dtype -> (C entry, columns of a 16-byte unit as a power of two)
_LAYER_TABLE = {
    torch.float32: ("fa_fedavg_f32_layers", 2),
    torch.bfloat16: ("fa_fedavg_bf16_layers", 3),
    torch.float16: ("fa_fedavg_f16_layers", 3),
    torch.float64: ("fa_fedavg_f64_layers", 1),
    # the plan counts output elements (doubles): four int32 / two int64 columns per 16-byte unit
    torch.int32: ("fa_fedavg_i32_layers", 2),
    torch.int64: ("fa_fedavg_i64_layers", 1),
}
_shape_of = operator.attrgetter("shape")
_cu_counts: dict = {}


def _cus(dev: torch.device) -> int:
    k = dev.index if dev.index is not None else torch.cuda.current_device()
    n = _cu_counts.get(k)
    if n is None:
        n = _cu_counts[k] = int(torch.cuda.get_device_properties(k).multi_processor_count)
    return n


def layer_plan(cols: Sequence[int], aligned: Sequence[bool], unit_lg: int, cus: int, units: int = 0):
    """fa_layers_plan, the host planner of the layer-table folds (no GPU):
    (plan, tiles, elems, units) with plan an [L, 4] int64 array of (cols,
    offset, tile0, aligned) rows.  units = 0 applies the rule (the most of 4,
    2, 1 units per lane whose balanced grid over the model's tiles covers 7/8
    of `cus` compute units, else 1); 1, 2 or 4 plans for that many."""
    L = len(cols)
    c = np.ascontiguousarray(cols, dtype=np.int64)
    al = np.ascontiguousarray(aligned, dtype=np.int32)
    plan = np.zeros((L, 4), dtype=np.int64)
    tiles, elems, u = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    _lib.call("fa_layers_plan", c.ctypes.data, al.ctypes.data, L, unit_lg, cus, units, plan.ctypes.data,
              ctypes.addressof(tiles), ctypes.addressof(elems), ctypes.addressof(u))
    return plan, tiles.value, elems.value, u.value


def mx_layer_plan(cols: Sequence[int], aligned: Sequence[bool]):
    """fa_mx_layers_plan, the host planner of the MX layer tables (no GPU):
    (plan, tiles, elems) with plan an [L, 4] int64 array of (cols, offset,
    tile0, aligned) rows.  cols are logical columns; tile0 counts WAVE tiles:
    ceil(ceil(cols / 32) / 64) per aligned layer, ceil(cols / 64) per layer
    with a data row off 16-B alignment."""
    L = len(cols)
    c = np.ascontiguousarray(cols, dtype=np.int64)
    al = np.ascontiguousarray(aligned, dtype=np.int32)
    plan = np.zeros((L, 4), dtype=np.int64)
    tiles, elems = ctypes.c_int64(), ctypes.c_int64()
    _lib.call("fa_mx_layers_plan", c.ctypes.data, al.ctypes.data, L, plan.ctypes.data, ctypes.addressof(tiles),
              ctypes.addressof(elems))
    return plan, tiles.value, elems.value


def plan_at_units(host_plan: np.ndarray, elems: int, unit_lg: int, cus: int, units: int):
    """The layers of `host_plan` (a layer_plan result) planned again at `units`
    units per lane: (plan, tiles).  Only tile0 may differ: a layer's offset is
    its predecessors' columns rounded up to 64 elements, whatever the tiling,
    so results split by the first plan's offsets stay valid.  No GPU."""
    plan, tiles, e, u = layer_plan(host_plan[:, 0], host_plan[:, 3], unit_lg, cus, units)
    assert u == units and e == elems and np.array_equal(plan[:, [0, 1, 3]], host_plan[:, [0, 1, 3]])
    return plan, tiles


class ModelRowSet:
    """N clients x L layers already on the GPU, prepared once for repeated
    one-launch folds (fold_model_rows): what RowSet is for one layer.

    parameters: N sequences of device tensors of one dtype and device;
    layers: the layer indices to take (default: every layer all clients have).
    Per layer the clients' tensors must be contiguous and of one shape
    (InvalidParameterShapeError otherwise).  Building the set gathers the L*N
    row bases, plans the tiles of all layers with the host planner
    (fa_layers_plan) and uploads table and plan in ONE copy; fold_model_rows
    then costs the factor upload and one kernel.  The set keeps the tensors
    alive; their CONTENTS may change between folds, their storage may not.

    An MX model: every client gives every layer as MXLayer(q, e, scale=None),
    all layers in ONE element format on one device; per layer every client
    carries a scale or none does, and within the set all layers carry scales
    or none does.  The set then holds the L*N data-row bases, the L*N scale-row
    bases, the optional L*N float32 scales and the wave-tile plan
    (fa_mx_layers_plan), uploaded in one copy, for fa_fedavg_mx_layers /
    fa_fedavg_mx_q_layers; shapes and sizes are the layers' LOGICAL ones (a
    float4 layer's last dimension doubled)."""

    mx = False  # an MX set (a set of plain tensors has no scale rows, scales or wave-tile plan)
    scale_rows = scales = dev_scales = scale_ptrs = None

    def __init__(self, parameters: Sequence[Sequence[torch.Tensor]], layers: Optional[Sequence[int]] = None):
        params = list(parameters)
        N = len(params)
        if N == 0:
            _lib.check(_lib.FA_ERR_NO_CLIENTS, "ModelRowSet")
        lis = list(range(min(map(len, params)))) if layers is None else list(layers)
        # one C-level pass per property and layer (as RowSet: no reshape per tensor)
        cols_of = [list(map(operator.itemgetter(li), params)) for li in lis]
        if any(isinstance(x, MXLayer) for col in cols_of for x in col):
            self._init_mx(cols_of, lis, N)
            return
        t0 = cols_of[0][0] if cols_of else None
        if t0 is not None and not (isinstance(t0, torch.Tensor) and t0.is_cuda):
            raise ValueError("layers must be CUDA (HIP) tensors")
        self.N, self.L, self.layers = N, len(lis), lis
        self.device = t0.device if t0 is not None else None
        self.dtype = t0.dtype if t0 is not None else None
        self.shapes, self.sizes = [], []
        host_ptrs = np.zeros((self.L, N), dtype=np.int64)
        for k, col in enumerate(cols_of):
            shp = col[0].shape
            if (set(map(_shape_of, col)) != {shp} or set(map(_dtype_of, col)) != {self.dtype}
                    or not all(map(torch.Tensor.is_contiguous, col))
                    or set(map(torch.Tensor.get_device, col)) != {t0.get_device()}):
                raise InvalidParameterShapeError(
                    f"layer {lis[k]}: all clients' tensors must be contiguous with one shape, dtype and device")
            self.shapes.append(tuple(shp))
            self.sizes.append(col[0].numel())
            host_ptrs[k] = np.fromiter(map(torch.Tensor.data_ptr, col), dtype=np.int64, count=N)
        self.tensors = cols_of  # keeps the storages alive
        self.host_ptrs = host_ptrs
        self.esize = t0.element_size() if t0 is not None else 0
        self.entry = None
        self._rowsets: dict = {}
        self._plans: dict = {}
        self.ptrs = self.plan = self.host_plan = None
        self.tiles = self.elems = self.units = 0
        if self.dtype in _LAYER_TABLE and self.L:
            self.entry, lg = _LAYER_TABLE[self.dtype]
            sizes = np.asarray(self.sizes, dtype=np.int64)
            aligned = ~((host_ptrs % 16) != 0).any(axis=1) | (sizes == 0)
            self.host_plan, self.tiles, self.elems, self.units = layer_plan(sizes, aligned, lg, _cus(self.device))
            both = torch.from_numpy(np.concatenate([host_ptrs.reshape(-1), self.host_plan.reshape(-1)])).to(self.device)
            self.ptrs, self.plan = both[:self.L * N], both[self.L * N:]
        self.offsets = [int(o) for o in self.host_plan[:, 1]] if self.host_plan is not None else []

    def _init_mx(self, cols_of: list, lis: list, N: int) -> None:
        """The tables of an MX model: validated as RowSet._mx_table validates one layer."""
        L = len(lis)
        m0 = cols_of[0][0]
        if not (isinstance(m0, MXLayer) and isinstance(m0.q, torch.Tensor) and m0.q.is_cuda):
            raise InvalidParameterShapeError("every client gives every layer of an MX model as an MXLayer of CUDA (HIP) "
                                             "tensors")
        dt, dev = m0.q.dtype, m0.q.device
        if dt not in _MX_FORMATS:
            raise InvalidParameterShapeError(f"MX layers hold fp8 / float4_e2m1fn_x2 elements, got {dt}")
        self.mx = True
        self.N, self.L, self.layers, self.device, self.dtype = N, L, lis, dev, dt
        self.shapes, self.sizes, self.tensors, self.scale_rows = [], [], [], []
        self.esize, self.entry, self._rowsets, self._plans = 1, None, {}, {}
        ptrs = np.zeros((2, L, N), dtype=np.int64)
        scaled = []
        for k, col in enumerate(cols_of):
            if not all(isinstance(x, MXLayer) for x in col):
                raise InvalidParameterShapeError(f"layer {lis[k]}: every client gives an MXLayer or none does")
            qs, es = [x.q for x in col], [x.e for x in col]
            if not all(isinstance(q, torch.Tensor) for q in qs) or set(map(_dtype_of, qs)) != {dt}:
                raise InvalidParameterShapeError(f"layer {lis[k]}: the MX layers of one set fold in one format ({dt}), "
                                                 f"got {sorted({str(getattr(q, 'dtype', type(q))) for q in qs})}")
            shp = qs[0].shape
            if (set(map(_shape_of, qs)) != {shp} or not all(map(torch.Tensor.is_contiguous, qs))
                    or set(map(torch.Tensor.get_device, qs)) != {m0.q.get_device()}):
                raise InvalidParameterShapeError(
                    f"layer {lis[k]}: all clients' tensors must be contiguous with one shape, dtype and device")
            cols = _mx_cols(dt, qs[0].numel())
            nb = (cols + 31) // 32
            if any(map(_is_nvfp4, es)):
                raise InvalidParameterShapeError(f"layer {lis[k]}: NVFP4 layers (float8_e4m3fn block scales) have no "
                                                 "layer table: aggregate_layers folds each in a launch of its own")
            for i, e in enumerate(es):
                if not (isinstance(e, torch.Tensor) and e.dtype in _MX_SCALE_DTYPES):
                    raise InvalidParameterShapeError(f"layer {lis[k]}, client {i}: the scale row must hold E8M0 bytes "
                                                     f"(float8_e8m0fnu or uint8), got {getattr(e, 'dtype', type(e))}")
                if e.numel() != nb or not e.is_contiguous() or e.device != dev:
                    raise InvalidParameterShapeError(f"layer {lis[k]}, client {i}: {e.numel()} scale bytes for {cols} "
                                                     f"columns (one per 32: {nb}, contiguous, on {dev})")
            given = [x.scale is not None for x in col]
            if any(given) and not all(given):
                raise InvalidParameterShapeError(f"layer {lis[k]}: every client's MXLayer carries a scale or none does")
            scaled.append(all(given))
            # the logical shape: a float4 layer's last dimension doubled (a 0-dim one: its two columns)
            self.shapes.append(tuple(shp[:-1]) + (_mx_cols(dt, shp[-1]),) if len(shp) else () if cols == 1 else (cols,))
            self.sizes.append(cols)
            self.tensors.append(qs)
            self.scale_rows.append(es)
            ptrs[0, k] = np.fromiter(map(torch.Tensor.data_ptr, qs), dtype=np.int64, count=N)
            ptrs[1, k] = np.fromiter(map(torch.Tensor.data_ptr, es), dtype=np.int64, count=N)
        if any(scaled) and not all(scaled):
            raise InvalidParameterShapeError("within one MX set all layers carry client scales or none does "
                                             f"(layers with: {[li for li, c in zip(lis, scaled) if c]})")
        self.host_ptrs = ptrs
        self.ptrs = self.plan = self.host_plan = None
        self.tiles = self.elems = self.units = 0
        self.offsets = []
        if not L:
            return
        if scaled[0]:
            self.scales = np.array([[np.float32(x.scale) for x in col] for col in cols_of], dtype=np.float32)
        sizes = np.asarray(self.sizes, dtype=np.int64)
        aligned = ~((ptrs[0] % 16) != 0).any(axis=1) | (sizes == 0)
        self.host_plan, self.tiles, self.elems = mx_layer_plan(sizes, aligned)
        self.units = 1
        self.offsets = [int(o) for o in self.host_plan[:, 1]]
        parts = [ptrs.reshape(-1).view(np.uint8), self.host_plan.reshape(-1).view(np.uint8)]
        if self.scales is not None:
            parts.append(self.scales.reshape(-1).view(np.uint8))
        both = torch.from_numpy(np.concatenate(parts)).to(dev)  # ONE copy: bases, plan, scales
        n = 8 * L * N
        self.ptrs, self.scale_ptrs = both[:n].view(torch.int64), both[n:2 * n].view(torch.int64)
        self.plan = both[2 * n:2 * n + 32 * L].view(torch.int64)
        if self.scales is not None:
            self.dev_scales = both[2 * n + 32 * L:].view(torch.float32)

    def plan_for(self, units: int):
        """(device plan, tiles) of the set's layers at `units` units per lane:
        the set's own where its rule chose that many, else planned on first
        use, uploaded once and kept (the widening kinds fix their units)."""
        if units == self.units:
            return self.plan, self.tiles
        hit = self._plans.get(units)
        if hit is None:
            host, tiles = plan_at_units(self.host_plan, self.elems, _LAYER_TABLE[self.dtype][1], _cus(self.device), units)
            hit = self._plans[units] = (torch.from_numpy(host.reshape(-1)).to(self.device), tiles)
        return hit

    def overlaps(self, t: torch.Tensor) -> bool:
        """Does tensor t share a byte with any client tensor (an MX set: or scale row) of the set?"""
        if self.L == 0 or t.numel() == 0:
            return False
        lo = t.data_ptr()
        hi = lo + t.numel() * t.element_size()
        nbytes = (np.asarray(self.sizes, dtype=np.int64) * self.esize)[:, None]
        if self.mx:  # [2, L, N] bases: the data rows' bytes, then the scale rows'
            cols = np.asarray(self.sizes, dtype=np.int64)[:, None]
            nbytes = np.stack([cols // 2 if self.dtype == torch.float4_e2m1fn_x2 else cols, (cols + 31) // 32])
        return bool(np.any((self.host_ptrs < hi) & (lo < self.host_ptrs + nbytes)))

    def rowset(self, k: int) -> RowSet:
        """The k-th layer of the set as a RowSet over this set's own device
        table (no upload, so it also serves under a stream capture): the
        per-layer route of fold_model_rows."""
        rs = self._rowsets.get(k)
        if rs is None:
            rows = [t.reshape(-1) for t in self.tensors[k]]
            if self.mx:  # a table of its own: the 2N bases of one layer are not adjacent in the set's
                rs = RowSet(rows, block_scales=[e.reshape(-1) for e in self.scale_rows[k]])
            elif self.ptrs is None or self.sizes[k] == 0:
                rs = RowSet(rows)
            else:
                rs = RowSet.__new__(RowSet)
                rs.rows, rs.N, rs.P, rs.device, rs.dtype = rows, self.N, self.sizes[k], self.device, self.dtype
                rs.view = None
                rs.ptrs = self.ptrs[k * self.N:(k + 1) * self.N]
                rs.host_ptrs = self.host_ptrs[k]
                rs.aligned = bool(self.host_plan[k, 3])
            self._rowsets[k] = rs
        return rs

    def split(self, flat: torch.Tensor) -> List[torch.Tensor]:
        """The layers of a flat result, as views shaped like the layers."""
        return [flat[o:o + n].reshape(s) for o, n, s in zip(self.offsets, self.sizes, self.shapes)]


def layer_table_enabled() -> bool:
    """aggregate_layers folds a device group of two or more layers in one
    launch (fold_model_rows) unless FEDAVG_LAYER_TABLE=0 (read per call),
    which keeps one fold_rows per layer."""
    return os.environ.get("FEDAVG_LAYER_TABLE", "1") != "0"


def _layer_factors(dt: torch.dtype, weights, scores, total) -> Optional[Factors]:
    """The factors fold_rows would fold rows of dtype dt with, or None where
    it would leave the row table (numpy promotes the result)."""
    if dt == torch.float32:
        return f32_factors(weights, scores, total)
    if dt == torch.bfloat16:
        return Factors.weak_f32(weights, scores, total) or Factors(weights, scores, np.dtype(np.float32), total=total)
    if dt == torch.float16:
        return f16_factors(weights, scores, total)
    if dt in _INT_ROWS:
        return _int_factors(_TORCH_TO_NP[dt], weights, scores, total)
    return f64_factors(weights, scores, total)


def _fold_model_mx(ms: "ModelRowSet", weights, scores, out, total, want_bf16, out_bf16, out_format, out_mx, scales):
    """An MX model through the MX layer table (fa_fedavg_mx_layers, with
    out_format / out_mx fa_fedavg_mx_q_layers): one launch for all L layers,
    the factors (and scales= of this call) in ONE staged upload.  Everything is
    decided here on the host before the launch."""
    if torch.cuda.is_current_stream_capturing():
        raise InvalidParameterShapeError("the MX layer table does not run under stream capture "
                                         "(its factors and scales are staged by a copy the graph would not own)")
    N, L, dev, E = ms.N, ms.L, ms.device, ms.elems
    if L == 0:
        return []
    quant = out_format is not None or out_mx is not None
    bf16 = want_bf16 or out_bf16 is not None
    lg = 0
    if quant:
        if out_format is None:
            out_format = out_mx[0].dtype
        if out_format not in _MX_FORMATS:
            raise InvalidParameterShapeError("out_format must be float8_e4m3fn, float8_e5m2 or float4_e2m1fn_x2, got "
                                             f"{out_format}")
        if bf16:
            raise InvalidParameterShapeError("out_format gives an MX result: want_bf16 / out_bf16 do not go with it")
        if out_format == torch.float4_e2m1fn_x2:
            lg = 1
            for k, (n, shp) in enumerate(zip(ms.sizes, ms.shapes)):
                if n % 2 or (shp and shp[-1] % 2):
                    raise InvalidParameterShapeError(f"layer {ms.layers[k]}: a float4_e2m1fn_x2 result holds two columns "
                                                     f"per byte, pairs of the last dimension: shape {shp}")
    c = ms.dev_scales
    host_c = None
    if scales is not None:
        if len(scales) != L or any(len(cs) != N for cs in scales):
            raise InvalidParameterShapeError(f"scales= takes {L} sequences of {N} numbers, one per layer")
        host_c = np.array([[np.float32(x) for x in cs] for cs in scales], dtype=np.float32).reshape(-1)
    _check_out("out", out, torch.float32, E)
    _check_out("out_bf16", out_bf16, torch.bfloat16, E)
    nq, ne = E >> lg, E >> 5
    if out_mx is not None:
        q, e = out_mx
        if not (isinstance(q, torch.Tensor) and q.dtype == out_format and q.device == dev and q.is_contiguous()
                and q.numel() >= nq):
            raise InvalidParameterShapeError(f"out_mx[0] must be a contiguous {out_format} tensor of >= {nq} elements "
                                             f"on {dev}")
        if not (isinstance(e, torch.Tensor) and e.dtype in _MX_SCALE_DTYPES and e.device == dev and e.is_contiguous()
                and e.numel() >= ne):
            raise InvalidParameterShapeError(f"out_mx[1] must hold >= {ne} contiguous E8M0 bytes (float8_e8m0fnu or "
                                             f"uint8) on {dev}")

    def usable(t):  # the tables live in device memory: the library cannot see an alias
        return t is not None and t.data_ptr() % 16 == 0 and not ms.overlaps(t)

    dst, dstb = out, out_bf16
    out = out if usable(out) else None
    outb = out_bf16 if usable(out_bf16) else None
    if outb is None and bf16:
        outb = torch.empty(E, dtype=torch.bfloat16, device=dev)
    if out is None and (dst is not None or (outb is None and not quant) or want_bf16):
        out = torch.empty(E, dtype=torch.float32, device=dev)
    qf = ef = None
    if quant:
        if out_mx is not None and usable(out_mx[0]) and not ms.overlaps(out_mx[1]):
            qf, ef = out_mx[0].reshape(-1), out_mx[1].reshape(-1)
        else:
            qf = torch.empty(nq, dtype=torch.uint8, device=dev).view(out_format)
            ef = torch.empty(ne, dtype=torch.uint8, device=dev).view(torch.float8_e8m0fnu)
    f = Factors.weak_f32(weights, scores, total) or Factors(weights, scores, _F32, total=total)
    parts = [f.a] if f.s is None else [f.a, f.s]
    if host_c is not None:
        parts.append(host_c)
    staged = stage_factors(parts, dev)
    a, s = staged[0], (staged[1] if f.s is not None else None)
    if host_c is not None:
        c = staged[-1]
    args = [_MX_FORMATS[ms.dtype], ms.ptrs.data_ptr(), ms.scale_ptrs.data_ptr(), ms.plan.data_ptr(), L, N, ms.tiles,
            a.data_ptr(), _ptr(s), _ptr(c), float(f.div), _ptr(out)]
    if quant:
        _lib.call("fa_fedavg_mx_q_layers", *args, _MX_FORMATS[out_format], qf.data_ptr(), ef.data_ptr(), stream_ptr(dev))
    else:
        _lib.call("fa_fedavg_mx_layers", *args, _ptr(outb), stream_ptr(dev))
    folded = sum(1 for n in ms.sizes if n)  # the layers fold_rows would count
    stats["mx_table_folds"] += 1
    stats["mx_folds"] += folded
    if dst is not None and dst is not out:
        dst.reshape(-1)[:E].copy_(out)
        out = dst
    if dstb is not None and dstb is not outb:
        dstb.reshape(-1)[:E].copy_(outb)
        outb = dstb
    if quant:
        stats["mx_out_folds"] += folded
        if out_mx is not None and qf.data_ptr() != out_mx[0].data_ptr():
            out_mx[0].view(torch.uint8).reshape(-1)[:nq].copy_(qf.view(torch.uint8))
            out_mx[1].view(torch.uint8).reshape(-1)[:ne].copy_(ef.view(torch.uint8))
            qf, ef = out_mx[0].reshape(-1), out_mx[1].reshape(-1)
        res = []
        for o, n, shp in zip(ms.offsets, ms.sizes, ms.shapes):
            qshape = shp[:-1] + (shp[-1] >> lg,) if shp else ()
            res.append(MXLayer(qf[o >> lg:(o + n) >> lg].reshape(qshape), ef[o >> 5:(o >> 5) + (n + 31) // 32]))
        return res
    if want_bf16:
        return ms.split(out.reshape(-1)), ms.split(outb.reshape(-1))
    if out_bf16 is not None:
        return ms.split(outb.reshape(-1)) if out is None else (ms.split(out.reshape(-1)), ms.split(outb.reshape(-1)))
    return ms.split(out.reshape(-1))


def fold_model_rows(model, weights: Sequence, scores: Optional[Sequence] = None, *,
                    out: Optional[torch.Tensor] = None, total=None, want_bf16: bool = False,
                    out_bf16: Optional[torch.Tensor] = None, out_format: Optional[torch.dtype] = None,
                    out_mx=None, scales: Optional[Sequence[Sequence]] = None):
    """fold_rows over every layer of a device-resident model in ONE launch.

    model: a ModelRowSet (prepared once, reusable) or N lists of device
    tensors (a ModelRowSet is built for this call).  Returns a list of L
    tensors shaped like the layers: views of one flat result in which layer k
    starts at model.offsets[k], a multiple of 64 elements.  Each holds, bit for
    bit, what fold_rows gives for that layer alone, with fold_rows' factor
    rules per dtype (int32 / int64 layers: float64 results, int_row_factors'
    rules).  out / out_bf16: flat buffers of model.elems elements to
    fold into; want_bf16 / out_bf16 (bf16 layers): as fold_rows, a pair of
    lists (fp32 layers, RNE bf16 layers), or the bf16 list alone when only
    out_bf16 was given.  Factors that promote the whole fold (widen_factors)
    take the widening layer table, fa_fedavg_widen_layers: still one launch,
    over a plan at the kind's units per lane that the set keeps, the layers in
    the promoted dtype, out= a flat buffer of that dtype.  Where fold_rows
    would leave the row table (a fold numpy types term by term, a dtype
    without a table, FEDAVG_WIDEN=0 under promoting factors, a stream capture
    in progress) every layer goes through fold_rows on its own, over the set's
    own table and into fresh tensors (out / out_bf16 are refused there).

    An MX model (a ModelRowSet of MXLayers, or N lists of them) folds through
    the MX layer table, one launch (fa_fedavg_mx_layers): L float32 tensors in
    the layers' logical shapes; out= / want_bf16 / out_bf16 as for bf16 layers.
    scales=: L sequences of N numbers, each rounded as np.float32(scale),
    replace the set's own client scales for this call.  out_format (or out_mx =
    (q_flat, e_flat), flat buffers of model.elems elements' codes and
    model.elems / 32 scale bytes) quantises the result in the same launch
    (fa_fedavg_mx_q_layers) and returns L MXLayer(q, e): q in the layer's
    logical shape, the last dimension halved for a float4 result, e its
    ceil(size / 32) scale bytes, both views of the flat buffers (layer k's
    codes at offsets[k] elements, its scale bytes at offsets[k] / 32) and each
    a valid row of a further MX fold.  Refused before any launch
    (InvalidParameterShapeError): out_format with bf16 outputs, a float4 result
    of a layer of odd size, a stream capture in progress."""
    ms = model if isinstance(model, ModelRowSet) else ModelRowSet(model)
    N = ms.N
    if len(weights) != N or (scores is not None and len(scores) != N):
        raise InvalidParameterShapeError(f"{N} clients but {len(weights)} weights"
                                         + ("" if scores is None else f" / {len(scores)} scores"))
    if ms.mx:
        return _fold_model_mx(ms, weights, scores, out, total, want_bf16, out_bf16, out_format, out_mx, scales)
    if out_format is not None or out_mx is not None or scales is not None:
        raise InvalidParameterShapeError("out_format / out_mx / scales are for MX models (layers given as MXLayer)")
    bf16 = ms.dtype == torch.bfloat16
    if (out_bf16 is not None or want_bf16) and not bf16:
        raise InvalidParameterShapeError("want_bf16 / out_bf16 are for bfloat16 layers")
    f = kind = None
    if ms.entry is not None and not torch.cuda.is_current_stream_capturing():
        f = _layer_factors(ms.dtype, weights, scores, total)
        if f is None and ms.dtype in _TORCH_TO_NP:
            # numpy promotes the whole fold: the widening layer table, where a kernel converts these rows on load
            wf = widen_factors(_TORCH_TO_NP[ms.dtype], weights, scores, total)
            if wf is not None:
                kind, f = wf
    if f is None:
        if out is not None or out_bf16 is not None:
            raise InvalidParameterShapeError("out / out_bf16 need the layer-table route (no promotion, no capture)")
        res = [fold_rows(ms.rowset(k), weights, scores, total=total, want_bf16=want_bf16) for k in range(ms.L)]
        if want_bf16:
            return ([r[0].reshape(s) for r, s in zip(res, ms.shapes)],
                    [r[1].reshape(s) for r, s in zip(res, ms.shapes)])
        return [r.reshape(s) for r, s in zip(res, ms.shapes)]
    dev, E = ms.device, ms.elems
    res_dt = torch.float32 if bf16 else torch.float64 if ms.dtype in _INT_ROWS else ms.dtype
    if kind is not None:
        res_dt = _widen_out_dtype(kind)
    _check_out("out", out, res_dt, E)
    _check_out("out_bf16", out_bf16, torch.bfloat16, E)

    def usable(t):  # the table lives in device memory: the library cannot see an alias
        return t is not None and t.data_ptr() % 16 == 0 and not ms.overlaps(t)

    dst, dstb = out, out_bf16
    out = out if usable(out) else None
    outb = out_bf16 if usable(out_bf16) else None
    if outb is None and (want_bf16 or dstb is not None):
        outb = torch.empty(E, dtype=torch.bfloat16, device=dev)
    if out is None and (dst is not None or outb is None or want_bf16):
        out = torch.empty(E, dtype=res_dt, device=dev)
    a, s = f.to(dev)
    folded = sum(1 for n in ms.sizes if n)  # layers folded through a table, as fold_rows counts them
    if kind is not None:
        # the kind fixes the units per lane; the offsets are the set's own (plan_at_units), so split() holds
        units = widen_geometry(kind)[1]
        plan, tiles = ms.plan_for(units)
        _lib.call("fa_fedavg_widen_layers", kind, ms.ptrs.data_ptr(), plan.data_ptr(), ms.L, N, tiles, units,
                  a.data_ptr(), _ptr(s), float(f.div), out.data_ptr(), stream_ptr(dev))
        stats["widened_table_folds"] += 1
        stats["widened_row_folds"] += folded
        if dst is not None and dst is not out:
            dst.reshape(-1)[:E].copy_(out)
            out = dst
        return ms.split(out.reshape(-1))
    args = [ms.ptrs.data_ptr(), ms.plan.data_ptr(), ms.L, N, ms.tiles, ms.units, a.data_ptr(), _ptr(s)]
    if bf16:
        _lib.call(ms.entry, *args, float(f.div), _ptr(out), _ptr(outb), stream_ptr(dev))
    elif ms.dtype == torch.float16:
        _lib.call(ms.entry, *args, _half_bits(f.div), out.data_ptr(), stream_ptr(dev))
    else:
        _lib.call(ms.entry, *args, float(f.div), out.data_ptr(), stream_ptr(dev))
    stats["layer_table_folds"] += 1
    if ms.dtype == torch.float64:
        stats["rows64_folds"] += folded
    elif ms.dtype in _INT_ROWS:
        stats["rows_int_folds"] += folded
    elif ms.dtype != torch.float32:
        stats["rows16_folds"] += folded
    if dst is not None and dst is not out:
        dst.reshape(-1)[:E].copy_(out)
        out = dst
    if dstb is not None and dstb is not outb:
        dstb.reshape(-1)[:E].copy_(outb)
        outb = dstb
    if want_bf16:
        return ms.split(out.reshape(-1)), ms.split(outb.reshape(-1))
    if out_bf16 is not None:
        return ms.split(outb.reshape(-1)) if out is None else (ms.split(out.reshape(-1)), ms.split(outb.reshape(-1)))
    return ms.split(out.reshape(-1))


# ---------------------------------------------------------------------------
# per-layer (reference-shaped) aggregation
# ---------------------------------------------------------------------------
def _layer_meta(parameters, n_eff):
    L = min(len(p) for p in parameters[:n_eff])
    shapes, dtypes = [], []
    for li in range(L):
        ref = parameters[0][li]
        shp = tuple(ref.shape)
        dt, mixed = ref.dtype, False
        for ci in range(1, n_eff):
            x = parameters[ci][li]
            if tuple(x.shape) != shp:
                raise InvalidParameterShapeError(
                    f"layer {li}: client {ci} has shape {tuple(x.shape)}, client 0 has {shp}")
            mixed = mixed or x.dtype != dt
        shapes.append(shp)
        # numpy folds rows of several dtypes too (the stream variants put their float64
        # running model ahead of integer rows): such a layer carries its per-row dtypes
        dtypes.append(tuple(parameters[ci][li].dtype for ci in range(n_eff)) if mixed else dt)
    return L, shapes, dtypes


def _rows_route(dt, fp32_result: bool, w, sc, total, where: torch.device, dev) -> bool:
    """Does a group of device layers of dtype dt fold per layer through
    fold_rows' row tables (no stacked copy)?  fp32 layers whose result stays
    fp32; bf16 layers (always float32 factors); float16 layers whose result
    stays float16; float64 layers whose result stays float64; int32 / int64
    layers whose fold int_row_factors accepts (it raises numpy's OverflowError
    here, before any launch).  The 16-bit, float64 and integer groups only where the layers already lie on the device the fold
    was asked for (the stacked copy is what moves them).  With
    FEDAVG_WIDEN_ROWS=1 also a group numpy promotes as a whole, where a
    widening kernel converts its rows on load (widen_factors), under the
    conditions of the integer groups."""
    if dt == torch.float32 and fp32_result:
        return True
    d = torch.device(dev)
    here = where.type == d.type and where.index == (d.index if d.index is not None else torch.cuda.current_device())
    if dt == torch.bfloat16:
        return here
    capturing = torch.cuda.is_current_stream_capturing()
    if dt == torch.float64:
        return here and not capturing and result_dtype(_F64, w, sc, total) == _F64
    if dt in _INT_ROWS and here and not capturing and int_row_factors(_TORCH_TO_NP[dt], w, sc, total) is not None:
        return True
    if dt == torch.float16 and here and result_dtype(np.dtype(np.float16), w, sc, total) == np.float16:
        return True
    return (widen_rows_enabled() and here and not capturing and dt in _TORCH_TO_NP
            and widen_factors(_TORCH_TO_NP[dt], w, sc, total) is not None)


def _unwrap_scaled(parameters, n_eff):
    """aggregate_layers' parameters with every ScaledLayer replaced by its
    tensor, and {layer index: the clients' scales of that layer}; the
    parameters themselves and {} when no layer is wrapped."""
    if not any(isinstance(x, ScaledLayer) for p in parameters[:n_eff] for x in p):
        return parameters, {}
    L = min(len(p) for p in parameters[:n_eff])
    plain = [list(p[:L]) for p in parameters[:n_eff]]
    scales = {}
    for li in range(L):
        wrapped = [isinstance(p[li], ScaledLayer) for p in plain]
        if not any(wrapped):
            continue
        if not all(wrapped):
            raise InvalidParameterShapeError(f"layer {li}: every client gives a ScaledLayer or none does")
        scales[li] = [p[li].scale for p in plain]
        for p in plain:
            p[li] = p[li].q
    return plain, scales


def _unwrap_mx(parameters, n_eff):
    """aggregate_layers' parameters with every MXLayer replaced by its element
    tensor, and {layer index: (the clients' scale-byte tensors, their scales or
    None)}; the parameters themselves and {} when no layer is wrapped."""
    if not any(isinstance(x, MXLayer) for p in parameters[:n_eff] for x in p):
        return parameters, {}
    L = min(len(p) for p in parameters[:n_eff])
    plain = [list(p[:L]) for p in parameters[:n_eff]]
    mx = {}
    for li in range(L):
        wrapped = [isinstance(p[li], MXLayer) for p in plain]
        if not any(wrapped):
            continue
        if not all(wrapped):
            raise InvalidParameterShapeError(f"layer {li}: every client gives an MXLayer or none does")
        given = [p[li].scale is not None for p in plain]
        if any(given) and not all(given):
            raise InvalidParameterShapeError(f"layer {li}: every client's MXLayer carries a scale or none does")
        if len({p[li].q.dtype for p in plain}) != 1 or plain[0][li].q.dtype not in _MX_FORMATS:
            raise InvalidParameterShapeError(f"layer {li}: MX layers fold in one format, every client's alike; got "
                                             f"{sorted({str(p[li].q.dtype) for p in plain})}")
        if len({_is_nvfp4(p[li].e) for p in plain}) != 1:
            raise InvalidParameterShapeError(f"layer {li}: MX layers fold in one format, every client's alike; got MXFP4 "
                                             "(E8M0 scales) and NVFP4 (float8_e4m3fn scales)")
        mx[li] = ([p[li].e.reshape(-1) for p in plain], [p[li].scale for p in plain] if all(given) else None)
        for p in plain:
            p[li] = p[li].q
    return plain, mx


def _mx_group_here(parameters, layer_mx, n_eff, lis, dev) -> bool:
    """Do the MX layers `lis` take the MX layer table?  Every client's element
    tensor and scale row contiguous and on the device the fold was asked for
    (the per-layer route folds a layer wherever it lies)."""
    d = torch.device(dev)
    want = (d.type, d.index if d.index is not None else torch.cuda.current_device())
    for li in lis:
        for t in [parameters[i][li] for i in range(n_eff)] + list(layer_mx[li][0]):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
                    and (t.device.type, t.device.index) == want):
                return False
    return True


def _multi(devices) -> Optional[list]:
    """The device list of a multi-GPU call, or None for a one-GPU call."""
    if devices is None:
        return None
    from .multigpu import resolve_devices
    devs = resolve_devices(devices)
    return devs if len(devs) > 1 else None


def aggregate_layers(parameters: Sequence[Sequence], weights: Sequence, scores: Optional[Sequence] = None,
                     device: Optional[torch.device] = None, devices=None, *,
                     out_format: Optional[torch.dtype] = None) -> List:
    """Reference-shaped FedAvg / stall-aware aggregation.

    parameters: N clients x L layers (numpy arrays, or CUDA tensors).  Returns
    L outputs (numpy in -> numpy out, tensors in -> CUDA tensors out).  zip()
    truncation over clients/weights/scores and over layers is kept
    (fed_avg_aggregator.py:32-41); the divisor is the sum of ALL weights.
    Clients' layers must agree in shape; where their dtypes differ (the stream
    variants' float64 running model ahead of integer rows) the layer is folded
    as numpy types it, row by row (fold_plan).

    devices: several GPUs of this process (multigpu.py): host float32 layers
    are folded one column bucket per GPU, bit-identical to one GPU.  Other
    layer groups (device tensors, other dtypes) run on the first of them.

    Device fp8 layers (float8_e4m3fn, float8_e5m2) fold one layer at a time
    through their row table, where they lie; such a layer may be given as
    ScaledLayer(q, scale) by every client: client i's rows then count as
    q_i.to(float32) * np.float32(scale_i) (fold_stacked's scales=).  Device MX
    layers are given as MXLayer(q, e, scale=None) by every client and fold the
    same way (fa_fedavg_mx_ptrs); a float4 layer's result has its last
    dimension doubled.  Two or more MX layers of one format on the fold's
    device, contiguous, fold in ONE launch per sub-group (the layers with
    client scales, the layers without) through the MX layer table
    (fold_model_rows, fa_fedavg_mx_layers) unless FEDAVG_LAYER_TABLE=0 or a
    stream capture is in progress; a sub-group of one layer folds as a lone
    layer does; the same bits either way.

    out_format (float8_e4m3fn, float8_e5m2, float4_e2m1fn_x2): every layer
    must be a device fp8 or MX layer, and each comes back as MXLayer(q, e)
    quantised in its fold's launch (fold_stacked's out_format=): q in the
    layer's logical shape, the last dimension halved for a float4 result, e the
    ceil(size / 32) scale bytes of the flattened layer.
    """
    multi = _multi(devices)
    if multi is not None and device is None:
        device = multi[0]
    elif devices is not None and multi is None and device is None:
        from .multigpu import resolve_devices
        device = resolve_devices(devices)[0]
    n_eff = min(len(parameters), len(weights), len(scores) if scores is not None else len(weights))
    if n_eff == 0:
        return []
    total_weights = list(weights)
    parameters, layer_scales = _unwrap_scaled(parameters, n_eff)
    parameters, layer_mx = _unwrap_mx(parameters, n_eff)
    L, shapes, dtypes = _layer_meta(parameters, n_eff)
    if L == 0:
        return []
    for li, dt in enumerate(dtypes):
        if dt == torch.float4_e2m1fn_x2 and li not in layer_mx:
            raise InvalidParameterShapeError(f"layer {li}: float4_e2m1fn_x2 rows fold only as MXLayers")
    for li in layer_scales:
        if dtypes[li] not in _FP8_FORMATS:
            raise InvalidParameterShapeError(f"layer {li}: a ScaledLayer holds fp8 rows, got {dtypes[li]}")
    for li, dt in enumerate(dtypes):
        if isinstance(dt, tuple) and any(d in _FP8_FORMATS for d in dt):
            raise InvalidParameterShapeError(f"layer {li}: fp8 rows fold only with rows of their own format, every "
                                             f"client's alike; got {sorted(set(map(str, dt)))}")
    on_device = isinstance(parameters[0][0], torch.Tensor)
    if out_format is not None:
        if out_format not in _MX_FORMATS:
            raise InvalidParameterShapeError("out_format must be float8_e4m3fn, float8_e5m2 or float4_e2m1fn_x2, got "
                                             f"{out_format}")
        for li, dt in enumerate(dtypes):
            if dt not in _MX_FORMATS or not (on_device and parameters[0][li].is_cuda):
                raise InvalidParameterShapeError(f"layer {li}: out_format is for device fp8 and MX layers, got {dt}")
    dev = device or (parameters[0][0].device if on_device else default_device())
    w = list(weights[:n_eff])
    sc = None if scores is None else list(scores[:n_eff])
    groups: dict = {}
    for li, dt in enumerate(dtypes):
        groups.setdefault(str(dt), []).append(li)
    outs: list = [None] * L
    for _, lis in groups.items():
        sizes = [int(np.prod(shapes[li])) if len(shapes[li]) else 1 for li in lis]
        P = sum(sizes)
        if dtypes[lis[0]] in _MX_FORMATS:
            # device fp8 layers: each folds from the clients' own bytes through its row table.  Two or more
            # MX layers on the fold's device: one table and one launch per sub-group (the layers with client
            # scales, the layers without; FEDAVG_LAYER_TABLE=0: a fold per layer); the same bits either way
            tabled = [li for li in lis if li in layer_mx and not _is_nvfp4(layer_mx[li][0][0])]  # NVFP4: no table
            if (len(tabled) >= 2 and layer_table_enabled() and not torch.cuda.is_current_stream_capturing()
                    and _mx_group_here(parameters, layer_mx, n_eff, tabled, dev)):
                folded = set()
                for sub in ([li for li in tabled if layer_mx[li][1] is None],
                            [li for li in tabled if layer_mx[li][1] is not None]):
                    if len(sub) < 2:  # a lone layer of its sub-group: the fold of one layer below
                        continue
                    folded.update(sub)
                    model = [[MXLayer(parameters[i][li], layer_mx[li][0][i],
                                      None if layer_mx[li][1] is None else layer_mx[li][1][i]) for li in sub]
                             for i in range(n_eff)]
                    for li, r in zip(sub, fold_model_rows(ModelRowSet(model), w, sc, total=sum(total_weights),
                                                          out_format=out_format)):
                        outs[li] = r
                lis = [li for li in lis if li not in folded]
            for li in lis:
                rows = [parameters[i][li].reshape(-1) for i in range(n_eff)]
                if li in layer_mx:
                    es, cs = layer_mx[li]
                    shp = shapes[li][:-1] + (_mx_cols(dtypes[li], shapes[li][-1]),) if shapes[li] else ()
                    res = fold_rows(rows, w, sc, total=sum(total_weights), scales=cs, block_scales=es,
                                    out_format=out_format)
                else:
                    shp = shapes[li]
                    res = fold_rows(rows, w, sc, total=sum(total_weights), scales=layer_scales.get(li),
                                    out_format=out_format)
                if out_format is None:
                    outs[li] = res.reshape(shp)
                elif out_format == torch.float4_e2m1fn_x2:
                    if not shp or shp[-1] % 2:
                        raise InvalidParameterShapeError(f"layer {li}: a float4_e2m1fn_x2 result packs pairs of the last "
                                                         f"dimension: shape {shp}")
                    outs[li] = MXLayer(res.q.reshape(shp[:-1] + (shp[-1] // 2,)), res.e)
                else:
                    outs[li] = MXLayer(res.q.reshape(shp), res.e)
            continue
        fp32_result = result_dtype(np.dtype(np.float32), total_weights, sc) == np.float32
        if isinstance(dtypes[lis[0]], tuple):
            # rows of several dtypes: one stacked matrix per run of rows of one dtype,
            # folded term by term as numpy types them
            rdts = dtypes[lis[0]]
            np_dts = [np.dtype(_TORCH_TO_NP.get(d, np.void) if on_device else d) for d in rdts]
            if any(d not in _NP_TO_TORCH for d in np_dts):
                raise InvalidParameterShapeError(f"layer {lis[0]}: unsupported row dtypes {sorted(set(map(str, rdts)))}")
            plan = fold_plan(np_dts, w, sc, sum(total_weights))
            segs, i = [], 0
            while i < n_eff:
                j = i + 1
                while j < n_eff and rdts[j] == rdts[i]:
                    j += 1
                segs.append(_stack_group(parameters[i:j], j - i, lis, sizes, P, dev, on_device))
                i = j
            res = _fold_general(segs, plan, w, sc, sum(total_weights))
        elif (not on_device and P > 0 and dtypes[lis[0]] == np.float16 and f16_stream_enabled() and
                result_dtype(np.dtype(np.float16), total_weights, sc) == np.float16):
            # host float16 rows whose result stays float16: the same pipe with
            # 2-byte rows, binary16 factors and the chunked binary16 fold
            # (fa_fold_f16), on one GPU
            res = _stream_group(parameters, n_eff, lis, P, w, sc, sum(total_weights), dev, np.float16)
        elif (not on_device and P > 0 and dtypes[lis[0]] == np.float64 and f64_stream_enabled() and
                result_dtype(_F64, total_weights, sc) == _F64):
            # host float64 rows whose result stays float64: the same pipe with
            # 8-byte rows, double factors and the chunked float64 fold
            # (fa_fold_f64), on one GPU
            res = _stream_group(parameters, n_eff, lis, P, w, sc, sum(total_weights), dev, np.float64)
        elif (not on_device and P > 0 and dtypes[lis[0]] == np.float32 and fp32_result):
            # host fp32 rows: pipelined pinned-chunk H2D + in-order chunked fold (bit-identical)
            if multi is not None:  # one column bucket per GPU, result assembled in pinned host memory
                flat = _stream_group_multi(parameters, n_eff, lis, P, w, sc, sum(total_weights), multi)
                off = 0
                for li, n in zip(lis, sizes):
                    outs[li] = flat[off:off + n].reshape(shapes[li])
                    off += n
                continue
            res = _stream_group(parameters, n_eff, lis, P, w, sc, sum(total_weights), dev)
        elif on_device and _rows_route(dtypes[lis[0]], fp32_result, w, sc, sum(total_weights),
                                       parameters[0][lis[0]].device, dev) and all(
                parameters[i][li].is_contiguous() for i in range(n_eff) for li in lis):
            # device fp32 / bf16 layers, float16 / float64 layers whose result stays in
            # their dtype, integer layers whose products stay in theirs, and (FEDAVG_WIDEN_ROWS=1) groups
            # promoted as a whole: fold each layer straight from the clients' own tensors
            # through a row-pointer list -- no stacking copy.  Two or more layers: one
            # table of every layer's rows and one launch (FEDAVG_LAYER_TABLE=0: a
            # fold per layer); the same bits either way
            if len(lis) >= 2 and layer_table_enabled() and not torch.cuda.is_current_stream_capturing():
                res = fold_model_rows(ModelRowSet(parameters[:n_eff], lis), w, sc, total=sum(total_weights))
                for li, r in zip(lis, res):
                    outs[li] = r
                continue
            for li in lis:
                rows = [parameters[i][li].reshape(-1) for i in range(n_eff)]
                outs[li] = fold_rows(rows, w, sc, total=sum(total_weights)).reshape(shapes[li])
            continue
        else:
            X = _stack_group(parameters, n_eff, lis, sizes, P, dev, on_device)
            res = fold_stacked(X, w, sc, total=sum(total_weights))
        flat = res if on_device else to_host(res)
        off = 0
        for li, n in zip(lis, sizes):
            outs[li] = flat[off:off + n].reshape(shapes[li])
            off += n
    return outs


# pinned staging per chunk; FEDAVG_STREAM_CHUNK_MB overrides.  The native pipe
# (ingest.NativeStreamingFold, round 3) keeps 3 chunks of 32 MB in flight: best
# or within the run-to-run spread of 16-64 MB x 3-6 slots on 10 x 582K, 100 x 1M,
# 100 x 10M and 1024 x 1M (profiles/r03_e2e_ramp/); the Python-driven
# StreamingFold (the direct-DMA route) keeps 2.
STREAM_CHUNK_BYTES = int(os.environ.get("FEDAVG_STREAM_CHUNK_MB", "32")) << 20
# DMA layers straight from page-locked documents instead of packing them
# (StreamingFold direct=True); FEDAVG_DIRECT_DMA=1 turns it on.
DIRECT_DMA = os.environ.get("FEDAVG_DIRECT_DMA", "0") == "1"


def _py_scalar(x) -> bool:
    return type(x) in (int, float)  # weak scalars: fp32 layers stay fp32 (NEP 50)


def f16_stream_enabled() -> bool:
    """Host float16 rows stream through the ingest pipe unless
    FEDAVG_F16_STREAM=0 (read per call), which keeps the materialised route:
    every row stacked into one pinned matrix, one H2D, one fa_fedavg_f16."""
    return os.environ.get("FEDAVG_F16_STREAM", "1") != "0"


def f64_stream_enabled() -> bool:
    """Host float64 rows stream through the ingest pipe unless
    FEDAVG_F64_STREAM=0 (read per call), which keeps the materialised route:
    every row stacked into one pinned matrix, one H2D, one fa_fedavg_f64."""
    return os.environ.get("FEDAVG_F64_STREAM", "1") != "0"


def _stream_dtype(layers, f64: bool = False) -> Optional[np.dtype]:
    """The dtype a row streams in: float32 or float16 -- and, where the caller
    has a float64 pipe to offer (f64: one GPU, FEDAVG_F64_STREAM not 0),
    float64 -- when every layer is a numpy array of that one dtype; None
    otherwise (mixed or other dtypes)."""
    dts = {x.dtype for x in layers if isinstance(x, np.ndarray)}
    if len(dts) != 1 or not all(isinstance(x, np.ndarray) for x in layers):
        return None
    dt = dts.pop()
    return dt if dt in (np.float32, np.float16) or (f64 and dt == np.float64) else None


def _fast_row(layers, shapes, dtype=np.float32) -> bool:
    """A row the streaming path can take: numpy layers of `dtype` (row 0's:
    float32, float16 or float64) shaped like row 0."""
    return (len(layers) == len(shapes) and
            all(isinstance(x, np.ndarray) and x.dtype == dtype and x.shape == shp
                for x, shp in zip(layers, shapes)))


def aggregate_decoded(items, scores: Optional[Sequence] = None, device: Optional[torch.device] = None,
                      devices=None, expected_rows: int = 0) -> List:
    """aggregate_layers over an iterator of decoded (layers, weight) rows, with
    the fold overlapping the decode.

    The strategies' aggregate() decodes every result and then folds
    (fed_avg_aggregator.py:64-92).  Here each host float32 row enters the
    pipelined StreamingFold as soon as it is decoded, so decoding row i+1
    overlaps the DMA of row i.  Same rows, same order, same factors: the result
    is bit-identical.  Rows whose layers are all float16 stream the same way
    through a float16 pipe (one GPU; FEDAVG_F16_STREAM=0 turns that off), and
    rows whose layers are all float64 through a float64 pipe (one GPU;
    FEDAVG_F64_STREAM=0 turns that off).
    Anything else (other or mixed dtypes, a row shaped or typed unlike row 0,
    weights that are not Python scalars, device tensors, nothing to fold)
    drains the iterator and runs aggregate_layers over every row, which is
    exactly the materialised path.  zip() truncation is kept: rows beyond
    len(scores) are not folded, their weights still count in the divisor.

    devices: several GPUs (multigpu.MultiStreamingFold): every GPU ingests and
    folds its own column bucket of each row, so the rows cross G PCIe links.
    expected_rows: the number of rows when the caller knows it (a list of
    results); the native pipe then shrinks its last chunks (a shorter tail).
    """
    multi = _multi(devices)
    if devices is not None and device is None:
        from .multigpu import resolve_devices
        device = resolve_devices(devices)[0]
    it = iter(items)
    first = next(it, None)
    if first is None:
        return []
    rows, weights = [first[0]], [first[1]]
    shapes = [getattr(x, "shape", None) for x in first[0]]
    n_fold = len(scores) if scores is not None else None
    # float64 rows stream on one GPU only, like float16 ones
    dt = _stream_dtype(first[0], f64=multi is None and f64_stream_enabled()) if len(shapes) > 0 else None
    if dt == np.float16 and (multi is not None or not f16_stream_enabled()):
        dt = None  # float16 rows stream on one GPU only
    fast = (dt is not None and _fast_row(first[0], shapes, dt) and _py_scalar(first[1]) and
            (scores is None or (len(scores) > 0 and all(_py_scalar(x) for x in scores))))
    P = sum(int(np.prod(shp)) if len(shp) else 1 for shp in shapes) if fast else 0
    if fast and P > 0:
        n_exp = min(expected_rows, n_fold) if n_fold is not None else expected_rows
        if multi is not None:
            from .multigpu import MultiStreamingFold
            sf = MultiStreamingFold(P, multi, chunk_bytes=STREAM_CHUNK_BYTES, direct=DIRECT_DMA,
                                    expected_rows=n_exp)
        else:
            from .ingest import make_streaming_fold
            sf = make_streaming_fold(P, device or default_device(), STREAM_CHUNK_BYTES, direct=DIRECT_DMA,
                                     expected_rows=n_exp, dtype=dt)
        sf.add(list(first[0]), first[1], None if scores is None else scores[0])
        for layers, w in it:
            rows.append(layers)
            weights.append(w)
            i = len(rows) - 1
            if not _py_scalar(w):
                break
            if n_fold is not None and i >= n_fold:
                continue
            if not _fast_row(layers, shapes, dt):
                break
            sf.add(list(layers), w, None if scores is None else scores[i])
        else:
            res = sf.finish(total=sum(weights))
            flat = res if multi is not None else to_host(res)
            outs, off = [], 0
            for shp in shapes:
                n = int(np.prod(shp)) if len(shp) else 1
                outs.append(flat[off:off + n].reshape(shp))
                off += n
            return outs
        sf.abandon()  # release the pipe now: no DMA or fold left running for GC to join
    for layers, w in it:
        rows.append(layers)
        weights.append(w)
    return aggregate_layers(rows, weights, scores, device=device, devices=devices)


def to_host(t: torch.Tensor) -> np.ndarray:
    """D2H of a result through page-locked memory (a pageable .cpu() ran at
    ~7 GB/s, pinned at PCIe rate).  The array views the pinned buffer and keeps
    it alive; the copy runs on the producing stream and is waited for here."""
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host.numpy()


def _stream_group(parameters, n, lis, P, w, sc, total, dev, dtype=np.float32) -> torch.Tensor:
    from .ingest import chunk_class, make_streaming_fold
    sf = make_streaming_fold(P, dev, chunk_class(max(1, n) * np.dtype(dtype).itemsize * P, STREAM_CHUNK_BYTES),
                             direct=DIRECT_DMA, expected_rows=n, dtype=dtype)
    for i in range(n):
        sf.add([parameters[i][li] for li in lis], w[i], None if sc is None else sc[i])
    return sf.finish(total=total)


def _stream_group_multi(parameters, n, lis, P, w, sc, total, devices) -> np.ndarray:
    from .multigpu import MultiStreamingFold
    sf = MultiStreamingFold(P, devices, chunk_bytes=STREAM_CHUNK_BYTES, direct=DIRECT_DMA, expected_rows=n)
    for i in range(n):
        sf.add([parameters[i][li] for li in lis], w[i], None if sc is None else sc[i])
    return sf.finish(total=total)


def _stack_group(parameters, n, lis, sizes, P, dev, on_device) -> torch.Tensor:
    ldx = ((P + ROW_ALIGN - 1) // ROW_ALIGN) * ROW_ALIGN
    stats["stacked_groups"] += 1
    if on_device:
        ref = parameters[0][lis[0]]
        X = torch.empty((n, ldx), dtype=ref.dtype, device=dev)
        for i in range(n):
            off = 0
            for li, sz in zip(lis, sizes):
                X[i, off:off + sz].copy_(parameters[i][li].reshape(-1))
                off += sz
        return X[:, :P]
    np_dt = np.asarray(parameters[0][lis[0]]).dtype
    tdt = _NP_TO_TORCH.get(np_dt)
    if tdt is None:
        raise InvalidParameterShapeError(f"unsupported parameter dtype {np_dt}")
    stage = torch.empty((n, ldx), dtype=tdt, pin_memory=True)
    sv = stage.numpy()
    for i in range(n):
        off = 0
        for li, sz in zip(lis, sizes):
            sv[i, off:off + sz] = np.asarray(parameters[i][li]).reshape(-1)
            off += sz
    X = torch.empty((n, ldx), dtype=tdt, device=dev)
    X.copy_(stage, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()  # stage may be freed after return
    return X[:, :P]
