"""lg_adam_step_rows and HipAdam.step(visible=) without a GPU: the declaration and its binding, the argument checks that come before
any device call, the row-index helpers of the kernel against integer division (CPU harness), and the run.py flag."""
import ctypes as C
import os
import re

import pytest

import adam_rows_common
import common
from lightgaussian_amd import _lib, optim, run as lg_run

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")
SPAN = _lib.ADAM_SPAN


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_symbol_declared_and_bound():
    src = _header()
    m = re.search(r"^int lg_adam_step_rows\((.*?)\);", src, flags=re.S | re.M)
    assert m, "lg_adam_step_rows is not declared in include/lightgaussian.h"
    assert len(m.group(1).split(",")) == 7
    assert "lg_adam_step_rows" in _lib.EXPORTS
    lib = _lib.load()
    assert len(lib.lg_adam_step_rows.argtypes) == 7 and lib.lg_adam_step_rows.restype is C.c_int
    body = re.search(r"typedef struct lg_adam_rows_tensor \{(.*?)\} lg_adam_rows_tensor;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z_0-9]+)\s*[;,]", body)
    assert fields == [f[0] for f in _lib.lg_adam_rows_tensor._fields_] == ["t", "row_mask", "rows"]
    assert _lib.lg_adam_rows_tensor._fields_[0][1] is _lib.lg_adam_tensor
    assert C.sizeof(_lib.lg_adam_rows_tensor) == 80 and C.sizeof(_lib.lg_adam_tensor) == 64


def test_abi_version_stays_7():
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", _header()).group(1)) == 7
    assert _lib.ABI_VERSION == 7 and _lib.load().lg_abi_version() == 7


def _tensor(numel=16, step=1, ptr=0x1000, mask=0x2001, rows=4, **kw):
    e = _lib.lg_adam_rows_tensor()
    e.t.param, e.t.grad, e.t.exp_avg, e.t.exp_avg_sq = (kw.get(k, ptr) for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
    e.t.numel, e.t.lr, e.t.weight_decay, e.t.step = numel, 1e-3, 0.0, step
    e.row_mask, e.rows = mask, rows
    return e


def _call(tensors, n=None, beta1=0.9, beta2=0.999):
    arr = (_lib.lg_adam_rows_tensor * max(len(tensors), 1))(*tensors)
    return _lib.load().lg_adam_step_rows(len(tensors) if n is None else n, arr, beta1, beta2, 1e-8, 0, None)


@pytest.mark.parametrize("what, kwargs", [
    ("numel", dict(tensors=[_tensor(numel=-1)])),
    ("step", dict(tensors=[_tensor(step=0)])),
    ("null", dict(tensors=[_tensor(param=None)])),
    ("null", dict(tensors=[_tensor(grad=None)])),
    ("null", dict(tensors=[_tensor(exp_avg=None)])),
    ("null", dict(tensors=[_tensor(exp_avg_sq=None)])),
    ("null", dict(tensors=[_tensor(numel=0, param=None), _tensor(grad=None, mask=None)])),     # the second entry is looked at too
    ("aligned", dict(tensors=[_tensor(param=0x1002)])),
    ("betas", dict(tensors=[_tensor()], beta1=1.0)),
    ("betas", dict(tensors=[_tensor()], beta1=-0.1)),
    ("betas", dict(tensors=[_tensor()], beta2=1.0)),
    ("betas", dict(tensors=[_tensor()], beta2=float("nan"))),
    ("num_tensors", dict(tensors=[_tensor()], n=-1)),
    ("rows < 1", dict(tensors=[_tensor(rows=0)])),
    ("rows < 1", dict(tensors=[_tensor(rows=-3)])),
    ("multiple of rows", dict(tensors=[_tensor(numel=16, rows=5)])),
    ("multiple of rows", dict(tensors=[_tensor(mask=None, rows=0), _tensor(numel=16, rows=32)])),   # after a dense entry, whose rows is not looked at
])
def test_invalid_arguments_refused_before_any_device_call(what, kwargs):
    """This process has no GPU: a call that reached the HIP runtime would come back as LG_ERR_DEVICE."""
    assert _call(**kwargs) == _lib.LG_ERR_INVALID_ARGUMENT
    msg = _lib.load().lg_last_error().decode()
    assert "lg_adam_step_rows" in msg and what in msg


def test_nothing_to_do_is_ok_without_a_device():
    assert _call([]) == _lib.LG_OK
    assert _call([_tensor(numel=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None, rows=0)]) == _lib.LG_OK
    assert _call([_tensor(numel=0, mask=None), _tensor(numel=0, rows=7)]) == _lib.LG_OK


# ---- the row of an element (lg_adam_rows.h) against integer division --------------------------------------------------------------

BIG_ROW_LENS = [4095, 4096, 4097, 65535, 65536, 2 ** 20 + 1, 2 ** 31 - 1]


def test_harness_is_built_for_the_librarys_span():
    assert adam_rows_common.harness().h_adam_span() == SPAN == optim.SPAN


def test_local_row_every_offset_for_row_len_1_to_300():
    """x = rem + k with rem < row_len and k < SPAN: every x in [0, row_len + SPAN)."""
    h = adam_rows_common.harness()
    bad = C.c_uint64(0)
    for row_len in range(1, 301):
        assert h.h_adam_local_rows(row_len, 0, 0, C.byref(bad)) == 0, f"row_len {row_len}: x = {bad.value}"


@pytest.mark.parametrize("row_len", BIG_ROW_LENS)
def test_local_row_large_rows(row_len):
    """Every x in [0, row_len + SPAN) up to 2^20 + 1; for the longer rows the first 2^16 offsets, 2^16 around the row's end, and the
    last SPAN + 2^16 the kernel can form."""
    h = adam_rows_common.harness()
    bad = C.c_uint64(0)
    if row_len <= 2 ** 20 + 1:
        assert h.h_adam_local_rows(row_len, 0, 0, C.byref(bad)) == 0, f"x = {bad.value}"
    else:
        end = row_len + SPAN
        for lo, hi in ((0, 2 ** 16), (row_len - 2 ** 15, row_len + 2 ** 15), (end - SPAN - 2 ** 16, end)):
            assert h.h_adam_local_rows(row_len, lo, hi, C.byref(bad)) == 0, f"x = {bad.value}"


def test_first_row_of_a_span_up_to_the_largest_base():
    """base = span * SPAN for spans up to 2^31 - 1 (the API's limit): first row and remainder, and through them the row of the span's
    first, middle and last element, against Python's integers."""
    h = adam_rows_common.harness()
    spans = [0, 1, 2, 3, 44, 45, 46, 1000, 2 ** 16, 2 ** 20 + 7, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1]
    rem = C.c_uint32(0)
    for row_len in [1, 2, 3, 4, 5, 7, 45, 48, 59, 300, 4095, 4096, 4097] + BIG_ROW_LENS:
        for span in spans:
            base = span * SPAN
            assert h.h_adam_first_row(span, row_len, C.byref(rem)) == base // row_len and rem.value == base % row_len, (row_len, span)
            for k in (0, 1, 2, 3, SPAN // 2, SPAN - 2, SPAN - 1):
                assert h.h_adam_row_of(span, k, row_len) == (base + k) // row_len, (row_len, span, k)


# ---- run.py ------------------------------------------------------------------------------------------------------------------------

def _script(tmp_path):
    script = tmp_path / "trainer.py"
    script.write_text("raise AssertionError('the script must not run')\n")
    return str(script)


def test_flag_parses(tmp_path):
    """--hip-adam=visible is taken as an option of the runner: what is refused is the script that does not exist."""
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--hip-adam=visible", str(tmp_path / "missing.py")])
    assert "does not exist" in str(e.value) and "unknown option" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--hip-adam=visibel", _script(tmp_path)])
    assert "unknown option" in str(e.value)


def test_visible_excludes_fused_adam_and_distributed(tmp_path):
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--hip-adam=visible", "--fused-adam", _script(tmp_path)])
    assert "--hip-adam=visible" in str(e.value) and "--fused-adam" in str(e.value)
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--distributed", "--hip-adam=visible", _script(tmp_path)])
    assert "--hip-adam=visible" in str(e.value) and "--distributed" in str(e.value)


def test_usage_and_docstring_list_the_flag(tmp_path):
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--no-such-flag", _script(tmp_path)])
    assert "--hip-adam=visible" in str(e.value)
    assert "--hip-adam=visible" in lg_run.__doc__
    assert "visible=" in optim.__doc__


def test_hook_takes_the_visible_mode_and_restores():
    import torch
    orig = torch.optim.Adam.__init__
    try:
        lg_run.hip_adam(True, visible=True)
        assert torch.optim.Adam.__init__ is not orig
        p = torch.nn.Parameter(torch.ones(5))
        opt = torch.optim.AdamW([p], lr=0.1)                    # CPU parameters: left alone, in this mode too
        assert type(opt) is torch.optim.AdamW and "step" not in opt.__dict__
    finally:
        lg_run.hip_adam(False)
    assert torch.optim.Adam.__init__ is orig
