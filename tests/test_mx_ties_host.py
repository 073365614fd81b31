"""The tie input of the MX quantiser (tests/mx_cases.py), checked on the CPU:
its reference quotients -- the committed float32 oracle over the rows
dequantised on the CPU -- cover every rounding boundary of each result format,
the contract in numpy (test_gpu_mx_out.py's _quantise) agrees on them with a
second reference written from the formats' definitions, and every deliberately
wrong quantiser differs from the contract on them.  tests/test_gpu_mx_ties.py
runs the same bytes through the kernels.
"""
import numpy as np
import pytest

import mx_cases as C
import test_gpu_fp8 as F8
import test_gpu_mx as M
import test_gpu_mx_out as MQ

FMTS = ["e4m3", "e5m2", "e2m1"]


def _quotients(fmt, source):
    if source == "mx":
        q, E, w = C.tie_mx_rows(fmt)
        return M._oracle("e5m2", q, E, w, None, None)[0]
    b, scales, w = C.tie_fp8_rows(fmt)
    return F8._oracle("e5m2", b, w, None, scales)[0]


def test_format_tables_are_the_formats():
    torch = pytest.importorskip("torch")
    for fmt, dt in (("e4m3", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2)):
        m = C.magnitudes(fmt)
        assert np.array_equal(torch.arange(m.size, dtype=torch.uint8).view(dt).to(torch.float64).numpy(), m)
        assert m[-1] == MQ.QF[fmt][1]
        assert not np.isfinite(torch.tensor([m.size], dtype=torch.uint8).view(dt).float().numpy()).any()
    assert np.array_equal(C.magnitudes("e2m1"), MQ.MAGS) and np.array_equal(C.magnitudes("e2m1"), M.E2M1[:8])


@pytest.mark.parametrize("source", ["mx", "fp8"])
@pytest.mark.parametrize("fmt", FMTS)
def test_quotients_are_the_targets_and_cover_every_boundary(fmt, source):
    v = _quotients(fmt, source)
    assert np.array_equal(v.view(np.uint32), C.tie_pieces(fmt)[1].view(np.uint32))  # the construction is exact
    assert C.tie_coverage(v, fmt) == list(C.TIE_E)
    # what coverage means for the codes: every finite code of the format is the answer somewhere, in both
    # signs, and at each midpoint the even code is
    q, _ = C.quantise(v, fmt)
    codes = np.stack([q & 15, q >> 4], -1).reshape(-1) if fmt == "e2m1" else q
    n, sign = C.magnitudes(fmt).size, 8 if fmt == "e2m1" else 128
    assert set(range(n)) | set(range(sign, sign + n)) <= set(codes.tolist())


@pytest.mark.parametrize("fmt", FMTS)
def test_the_two_references_agree(fmt):
    v = _quotients(fmt, "mx")
    q1, e1 = MQ._quantise(v, fmt)
    q2, e2 = C.quantise(v, fmt)
    assert np.array_equal(e1, e2) and np.array_equal(q1, q2)
    # ... and on dead blocks, zeros, float32 subnormals and values past the clamp
    rng = np.random.default_rng(5)
    u = (rng.standard_normal(32 * 40) * np.exp2(rng.integers(-140, 60, 32 * 40))).astype(np.float32)
    u[3], u[40], u[70:96], u[100] = np.nan, np.inf, 0.0, -0.0
    q1, e1 = MQ._quantise(u, fmt)
    q2, e2 = C.quantise(u, fmt)
    assert np.array_equal(e1, e2) and np.array_equal(q1, q2) and e2[0] == e2[1] == 255 and not q2[:32].any()


@pytest.mark.parametrize("name", list(C.WRONG))
@pytest.mark.parametrize("fmt", FMTS)
def test_every_wrong_quantiser_differs_on_the_tie_input(fmt, name):
    kw, fmts = C.WRONG[name]
    if fmt not in fmts:
        with pytest.raises(AssertionError, match="no code past maxnorm"):
            C.quantise(np.zeros(32, dtype=np.float32), fmt, **kw)
        return
    v = _quotients(fmt, "mx")
    q, e = C.quantise(v, fmt)
    wq, we = C.quantise(v, fmt, **kw)
    differs = int((q != wq).sum()) + int((e != we).sum())
    print(f"{fmt}, {name}: {differs} bytes differ")
    assert differs > 0
    if name == "E from amax rounded up":
        assert (e != we).any()
    else:
        assert np.array_equal(e, we) and (q != wq).any()
