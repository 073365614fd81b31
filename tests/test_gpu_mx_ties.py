"""The MX quantiser of the folds at every rounding boundary: the tie input of
tests/mx_cases.py (every midpoint of the result format with its float32
neighbours in both signs, the clamp, the block-exponent boundary, at two block
exponents) through the MX pitched vector path, the MX one-column path, an fp8
source, the layer table and every form of the bench library's
fa_fedavg_mx_q_form.  The quotients are the committed float32 oracle's over the
rows dequantised on the CPU; the expected bytes are mx_cases.quantise's, the
reference written from the formats' definitions (tests/test_mx_ties_host.py
pins it to test_gpu_mx_out.py's _quantise and shows what the input tells
apart).  Codes and scale bytes are compared as bytes; no tolerance.
"""
import functools

import numpy as np
import pytest

import mx_cases as C
import test_gpu_fp8 as F8
import test_gpu_mx as M
import test_gpu_mx_out as MQ
from fedlesscan_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMTS = M.FMTS
OUT_ID = {"e4m3": _lib.FA_MX_E4M3, "e5m2": _lib.FA_MX_E5M2, "e2m1": _lib.FA_MX_E2M1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _expect(out, source="mx"):
    """(float32 quotients, their bf16 bits), (code bytes, scale bytes) of the tie input of format `out`."""
    if source == "mx":
        q, E, w = C.tie_mx_rows(out)
        exp = M._oracle("e5m2", q, E, w, None, None)
    else:
        b, scales, w = C.tie_fp8_rows(out)
        exp = F8._oracle("e5m2", b, w, None, scales)
    assert C.tie_coverage(exp[0], out) == list(C.TIE_E)
    ref = C.quantise(exp[0], out)
    mq = MQ._quantise(exp[0], out)
    assert np.array_equal(ref[0], mq[0]) and np.array_equal(ref[1], mq[1])
    return exp, ref


def _same_bytes(got, ref, what):
    gq, ge = got.q.view(torch.uint8).cpu().numpy().reshape(-1), got.e.view(torch.uint8).cpu().numpy().reshape(-1)
    assert gq.shape == ref[0].shape and ge.shape == ref[1].shape, what
    bad = np.flatnonzero(ge != ref[1])
    assert bad.size == 0, f"{what}: {bad.size} scale bytes differ, first {bad[:4]}: {ge[bad[:4]]} != {ref[1][bad[:4]]}"
    bad = np.flatnonzero(gq != ref[0])
    assert bad.size == 0, f"{what}: {bad.size} code bytes differ, first {bad[:4]}: {gq[bad[:4]]} != {ref[0][bad[:4]]}"


@pytest.mark.parametrize("layout", ["pitched", "table", "table_odd_row"])
@pytest.mark.parametrize("out", list(FMTS))
def test_mx_source(dev, out, layout):
    """The pitched and table vector paths, and the one-column path (a row a byte off)."""
    exp, ref = _expect(out)
    q, E, w = C.tie_mx_rows(out)
    f32 = torch.zeros(q.shape[1], dtype=torch.float32, device=dev)
    got = M._fold("e5m2", q, E, layout, dev, w, out_format=FMTS[out], out=f32)
    _same_bytes(got, ref, f"-> {out}, {layout}")
    M._same(f32, exp, "out=")


@pytest.mark.parametrize("layout", ["stacked", "table", "table_odd_row"])
@pytest.mark.parametrize("out", list(FMTS))
def test_fp8_source(dev, out, layout):
    """A block is two lanes' units; the same quotients from plain e5m2 rows with per-client scales."""
    exp, ref = _expect(out, "fp8")
    assert np.array_equal(exp[0].view(np.uint32), _expect(out)[0][0].view(np.uint32))
    b, scales, w = C.tie_fp8_rows(out)
    got = F8._fold(F8._rows(b, "e5m2", layout, dev), w, scales=scales, out_format=FMTS[out])
    _same_bytes(got, ref, f"fp8 -> {out}, {layout}")


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("out", list(FMTS))
def test_layer_table(dev, out, odd):
    """The input as one layer between two others (odd: its middle data row a byte off, the one-column path)."""
    from fedlesscan_amd import MXLayer, engine
    exp, ref = _expect(out)
    q, E, w = C.tie_mx_rows(out)
    data = [M._bytes("e5m2", 4, 70), (q, E), M._bytes("e5m2", 4, 38)]
    cols = []
    for k, (lq, lE) in enumerate(data):
        rows = M._place(lq, "table_odd_row" if odd and k == 1 else "table", dev, FMTS["e5m2"], 16)
        cols.append([MXLayer(r, e) for r, e in zip(rows, M._place(lE, "table_odd_row", dev, torch.float8_e8m0fnu, 3))])
    ms = engine.ModelRowSet([[col[i] for col in cols] for i in range(4)])
    assert ms.host_plan[:, 3].tolist() == [1, int(not odd), 1]
    before = engine.stats["mx_table_folds"]
    got = engine.fold_model_rows(ms, w, out_format=FMTS[out])
    assert engine.stats["mx_table_folds"] == before + 1
    _same_bytes(got[1], ref, f"layer table -> {out}")
    for k in (0, 2):
        MQ._same_mx(got[k], M._oracle("e5m2", *data[k], w, None, None)[0], out, f"layer {k}")


@pytest.mark.parametrize("form", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("out", list(FMTS))
def test_bench_forms_give_the_products_bytes(dev, out, form):
    """fa_fedavg_mx_q_form: the multiply and sign-patching forms of the epilogue beside the product's."""
    from fedlesscan_amd import MXLayer, engine
    exp, ref = _expect(out)
    q, E, w = C.tie_mx_rows(out)
    P, B = q.shape[1], _lib.load_bench()
    X, S = torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(np.array(E)).to(dev)
    assert X.data_ptr() % 16 == 0 and P % 16 == 0
    a = torch.tensor(np.array(w, dtype=np.float32), device=dev)
    f32 = torch.zeros(P, dtype=torch.float32, device=dev)
    oq = torch.zeros(P // 2 if out == "e2m1" else P, dtype=torch.uint8, device=dev)
    oe = torch.zeros(P // 32, dtype=torch.uint8, device=dev)
    _lib.check(B.fa_fedavg_mx_q_form(_lib.FA_MX_E5M2, X.data_ptr(), S.data_ptr(), 4, P, P, P // 32, a.data_ptr(),
                                     float(sum(w)), f32.data_ptr(), OUT_ID[out], oq.data_ptr(), oe.data_ptr(),
                                     engine.stream_ptr(dev), form), "fa_fedavg_mx_q_form", bench=True)
    _same_bytes(MXLayer(oq, oe), ref, f"form {form} -> {out}")
    M._same(f32, exp, f"form {form}: out_f32")
