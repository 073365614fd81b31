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
                 exact: bool = True, out_bf16: Optional[torch.Tensor] = None):
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
    """
    N, P, ldx = _check_matrix(X)
    if len(weights) != N or (scores is not None and len(scores) != N):
        raise InvalidParameterShapeError(f"{N} rows but {len(weights)} weights"
                                         + ("" if scores is None else f" / {len(scores)} scores"))
    dev = X.device
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
_ROW_TABLE_DTYPES = (torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int32, torch.int64)
_INT_ROWS = {torch.int32: "fa_fedavg_i32_ptrs", torch.int64: "fa_fedavg_i64_ptrs"}
# dtypes whose row-table fold does not run under a stream capture: they keep the route they had before it
_NO_CAPTURE_TABLE = (torch.float64, torch.int32, torch.int64)
# process-wide route counters (diagnostics, as StreamingFold.stats): 16-bit and
# float64 folds that ran through a row table (layers: a one-launch model fold
# counts each of its layers), layer groups copied into a stacked matrix,
# one-launch model folds (fa_fedavg_*_layers), integer folds that ran through a
# row table (counted as the float64 ones), promoted stacked folds that read
# the narrow rows (fa_fedavg_widen; nothing else counts there)
stats = {"rows16_folds": 0, "rows64_folds": 0, "stacked_groups": 0, "layer_table_folds": 0, "rows_int_folds": 0,
         "widened_folds": 0}


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
      - other bfloat16 / float16 / float64 rows get the same table for
        fa_fedavg_bf16_ptrs / fa_fedavg_f16_ptrs / fa_fedavg_f64_ptrs
        (`aligned` picks the kernels);
      - other int32 / int64 rows get the same table for fa_fedavg_i32_ptrs /
        fa_fedavg_i64_ptrs, which fold_rows takes where int_row_factors
        accepts the fold.
    fold_rows(rowset, weights) then costs the factor upload and the kernel.
    The RowSet keeps the tensors alive; their CONTENTS may change between
    folds, their storage may not (re-create the RowSet after reallocating)."""

    def __init__(self, rows: Sequence[torch.Tensor]):
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
        # (float64 and integer rows met under a stream capture keep the stacked copy they had before the row table)
        if dt in _ROW_TABLE_DTYPES and P > 0 and not (dt in _NO_CAPTURE_TABLE
                                                      and torch.cuda.is_current_stream_capturing()):
            host_ptrs = self.host_ptrs = np.fromiter(map(torch.Tensor.data_ptr, rows), dtype=np.int64, count=N)
            self.view = _equal_stride_view(rows, host_ptrs, P)
            if self.view is None:
                self.ptrs = torch.from_numpy(host_ptrs).to(dev)
                self.aligned = not (host_ptrs % 16).any()

    def overlaps(self, t: torch.Tensor) -> bool:
        """Does tensor t share a byte with any row?"""
        if self.host_ptrs is None or self.P == 0 or t.numel() == 0:
            return False
        lo = t.data_ptr()
        hi = lo + t.numel() * t.element_size()
        return bool(np.any((self.host_ptrs < hi) & (lo < self.host_ptrs + self.P * self.rows[0].element_size())))

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


def fold_rows(rows, weights: Sequence, scores: Optional[Sequence] = None, *,
              out: Optional[torch.Tensor] = None, total=None, want_bf16: bool = False,
              out_bf16: Optional[torch.Tensor] = None):
    """The fold over separately allocated 1-D CUDA rows (no stacking copy for
    fp32, bfloat16, float16 / float64 rows whose result stays in their dtype, and
    int32 / int64 rows whose products stay in their dtype: int_row_factors).  `rows` is a
    RowSet (prepared once, reusable) or a sequence of tensors (a RowSet is
    built for this call).  want_bf16 / out_bf16: as fold_stacked (bf16 rows)."""
    rs = rows if isinstance(rows, RowSet) else RowSet(rows)
    if len(weights) != rs.N or (scores is not None and len(scores) != rs.N):
        raise InvalidParameterShapeError(f"{rs.N} rows but {len(weights)} weights"
                                         + ("" if scores is None else f" / {len(scores)} scores"))
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
        # no row-table fold for this dtype / these factors (float16 rows under
        # numpy-scalar weights promote): the stacked fold, over the rows' own
        # storage when they sit at a fixed pitch, else over a stacked copy
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
    alive; their CONTENTS may change between folds, their storage may not."""

    def __init__(self, parameters: Sequence[Sequence[torch.Tensor]], layers: Optional[Sequence[int]] = None):
        params = list(parameters)
        N = len(params)
        if N == 0:
            _lib.check(_lib.FA_ERR_NO_CLIENTS, "ModelRowSet")
        lis = list(range(min(map(len, params)))) if layers is None else list(layers)
        # one C-level pass per property and layer (as RowSet: no reshape per tensor)
        cols_of = [list(map(operator.itemgetter(li), params)) for li in lis]
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

    def overlaps(self, t: torch.Tensor) -> bool:
        """Does tensor t share a byte with any client tensor of the set?"""
        if self.L == 0 or t.numel() == 0:
            return False
        lo = t.data_ptr()
        hi = lo + t.numel() * t.element_size()
        nbytes = (np.asarray(self.sizes, dtype=np.int64) * self.esize)[:, None]
        return bool(np.any((self.host_ptrs < hi) & (lo < self.host_ptrs + nbytes)))

    def rowset(self, k: int) -> RowSet:
        """The k-th layer of the set as a RowSet over this set's own device
        table (no upload, so it also serves under a stream capture): the
        per-layer route of fold_model_rows."""
        rs = self._rowsets.get(k)
        if rs is None:
            rows = [t.reshape(-1) for t in self.tensors[k]]
            if self.ptrs is None or self.sizes[k] == 0:
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


def fold_model_rows(model, weights: Sequence, scores: Optional[Sequence] = None, *,
                    out: Optional[torch.Tensor] = None, total=None, want_bf16: bool = False,
                    out_bf16: Optional[torch.Tensor] = None):
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
    out_bf16 was given.  Where fold_rows would leave the row table (factors
    that promote the result, a dtype without a table, a stream capture in
    progress) every layer goes through fold_rows on its own, over the set's
    own table and into fresh tensors (out / out_bf16 are refused there)."""
    ms = model if isinstance(model, ModelRowSet) else ModelRowSet(model)
    N = ms.N
    if len(weights) != N or (scores is not None and len(scores) != N):
        raise InvalidParameterShapeError(f"{N} clients but {len(weights)} weights"
                                         + ("" if scores is None else f" / {len(scores)} scores"))
    bf16 = ms.dtype == torch.bfloat16
    if (out_bf16 is not None or want_bf16) and not bf16:
        raise InvalidParameterShapeError("want_bf16 / out_bf16 are for bfloat16 layers")
    f = None
    if ms.entry is not None and not torch.cuda.is_current_stream_capturing():
        f = _layer_factors(ms.dtype, weights, scores, total)
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
    args = [ms.ptrs.data_ptr(), ms.plan.data_ptr(), ms.L, N, ms.tiles, ms.units, a.data_ptr(), _ptr(s)]
    if bf16:
        _lib.call(ms.entry, *args, float(f.div), _ptr(out), _ptr(outb), stream_ptr(dev))
    elif ms.dtype == torch.float16:
        _lib.call(ms.entry, *args, _half_bits(f.div), out.data_ptr(), stream_ptr(dev))
    else:
        _lib.call(ms.entry, *args, float(f.div), out.data_ptr(), stream_ptr(dev))
    stats["layer_table_folds"] += 1
    folded = sum(1 for n in ms.sizes if n)  # layers folded through a table, as fold_rows counts them
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
    was asked for (the stacked copy is what moves them)."""
    if dt == torch.float32:
        return fp32_result
    d = torch.device(dev)
    here = where.type == d.type and where.index == (d.index if d.index is not None else torch.cuda.current_device())
    if dt == torch.bfloat16:
        return here
    if dt == torch.float64:
        return (here and not torch.cuda.is_current_stream_capturing()
                and result_dtype(_F64, w, sc, total) == _F64)
    if dt in _INT_ROWS:
        return (here and not torch.cuda.is_current_stream_capturing()
                and int_row_factors(_TORCH_TO_NP[dt], w, sc, total) is not None)
    return dt == torch.float16 and here and result_dtype(np.dtype(np.float16), w, sc, total) == np.float16


def _multi(devices) -> Optional[list]:
    """The device list of a multi-GPU call, or None for a one-GPU call."""
    if devices is None:
        return None
    from .multigpu import resolve_devices
    devs = resolve_devices(devices)
    return devs if len(devs) > 1 else None


def aggregate_layers(parameters: Sequence[Sequence], weights: Sequence, scores: Optional[Sequence] = None,
                     device: Optional[torch.device] = None, devices=None) -> List:
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
    L, shapes, dtypes = _layer_meta(parameters, n_eff)
    if L == 0:
        return []
    on_device = isinstance(parameters[0][0], torch.Tensor)
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
            # their dtype, and integer layers whose products stay in theirs: fold each layer straight from the clients' own tensors
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
