"""lg_adam_step and lightgaussian_amd.optim without a GPU: the declaration and its binding, the argument checks that come before
any device call, the run.py hook and flag, and the refusal of CPU parameters."""
import ctypes as C
import os
import re

import pytest
import torch

import common
from lightgaussian_amd import _lib, optim, run as lg_run

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")


def _header():
    return open(HDR).read()


def test_symbol_declared_and_bound():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"^int lg_adam_step\((.*?)\);", src, flags=re.S | re.M)
    assert m, "lg_adam_step is not declared in include/lightgaussian.h"
    assert len(m.group(1).split(",")) == 7
    assert "lg_adam_step" in _lib.EXPORTS
    lib = _lib.load()
    assert len(lib.lg_adam_step.argtypes) == 7 and lib.lg_adam_step.restype is C.c_int
    body = re.search(r"typedef struct lg_adam_tensor \{(.*?)\} lg_adam_tensor;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z_0-9]+)\s*[;,]", body)
    assert fields == [f[0] for f in _lib.lg_adam_tensor._fields_]
    assert C.sizeof(_lib.lg_adam_tensor) == 64
    # the constants the Python side and the tests size their cases by are the header's
    assert int(re.search(r"#define LG_ADAM_MAX_TENSORS (\d+)", src).group(1)) == _lib.ADAM_MAX_TENSORS == optim.MAX_TENSORS >= 8
    assert int(re.search(r"#define LG_ADAM_SPAN (\d+)", src).group(1)) == _lib.ADAM_SPAN == optim.SPAN
    assert int(re.search(r"#define LG_ADAM_DECOUPLED_WD (\d+)u", src).group(1)) == _lib.ADAM_DECOUPLED_WD


def test_abi_version_stays_7():
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", _header()).group(1)) == 7
    assert _lib.ABI_VERSION == 7 and _lib.load().lg_abi_version() == 7


def _tensor(numel=16, step=1, ptr=0x1000, **kw):
    t = _lib.lg_adam_tensor()
    t.param, t.grad, t.exp_avg, t.exp_avg_sq = (kw.get(k, ptr) for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
    t.numel, t.lr, t.weight_decay, t.step = numel, 1e-3, 0.0, step
    return t


def _call(tensors, n=None, beta1=0.9, beta2=0.999):
    arr = (_lib.lg_adam_tensor * max(len(tensors), 1))(*tensors)
    return _lib.load().lg_adam_step(len(tensors) if n is None else n, arr, beta1, beta2, 1e-8, 0, None)


@pytest.mark.parametrize("what, kwargs", [
    ("numel", dict(tensors=[_tensor(numel=-1)])),
    ("step", dict(tensors=[_tensor(step=0)])),
    ("null", dict(tensors=[_tensor(param=None)])),
    ("null", dict(tensors=[_tensor(grad=None)])),
    ("null", dict(tensors=[_tensor(exp_avg=None)])),
    ("null", dict(tensors=[_tensor(exp_avg_sq=None)])),
    ("null", dict(tensors=[_tensor(numel=0, param=None), _tensor(grad=None)])),       # the second entry is looked at too
    ("betas", dict(tensors=[_tensor()], beta1=1.0)),
    ("betas", dict(tensors=[_tensor()], beta1=-0.1)),
    ("betas", dict(tensors=[_tensor()], beta2=1.0)),
    ("betas", dict(tensors=[_tensor()], beta2=float("nan"))),
    ("num_tensors", dict(tensors=[_tensor()], n=-1)),
])
def test_invalid_arguments_refused_before_any_device_call(what, kwargs):
    """This process has no GPU: a call that reached the HIP runtime would come back as LG_ERR_DEVICE."""
    assert _call(**kwargs) == _lib.LG_ERR_INVALID_ARGUMENT
    msg = _lib.load().lg_last_error().decode()
    assert "lg_adam_step" in msg and what in msg


def test_nothing_to_do_is_ok_without_a_device():
    assert _call([]) == _lib.LG_OK
    assert _call([_tensor(numel=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None)]) == _lib.LG_OK


def test_hip_adam_hook_leaves_cpu_optimizers_alone_and_restores():
    orig = torch.optim.Adam.__init__
    try:
        lg_run.hip_adam(True)
        hooked = torch.optim.Adam.__init__
        assert hooked is not orig
        lg_run.hip_adam(True)                                  # idempotent
        assert torch.optim.Adam.__init__ is hooked
        p = torch.nn.Parameter(torch.ones(5))
        opt = torch.optim.AdamW([{"params": [p], "lr": 0.1, "name": "xyz"}], lr=0.0, eps=1e-15)
        assert type(opt) is torch.optim.AdamW and not isinstance(opt, optim._HipStep)
        p.grad = torch.ones(5)
        opt.step()                                             # torch's own CPU step
        assert float(p.detach()[0]) < 1.0
    finally:
        lg_run.hip_adam(False)
    assert torch.optim.Adam.__init__ is orig
    lg_run.hip_adam(False)
    assert torch.optim.Adam.__init__ is orig


def test_hip_adam_and_fused_adam_exclude_each_other(tmp_path):
    script = tmp_path / "trainer.py"
    script.write_text("raise AssertionError('the script must not run')\n")
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--hip-adam", "--fused-adam", str(script)])
    assert "--hip-adam" in str(e.value) and "--fused-adam" in str(e.value)
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--no-such-flag", str(script)])
    assert "--hip-adam" in str(e.value)                        # the usage text lists the flag
    assert "--hip-adam" in lg_run.__doc__


@pytest.mark.parametrize("cls", [optim.HipAdam, optim.HipAdamW])
def test_cpu_parameters_raise(cls):
    p = torch.nn.Parameter(torch.ones(5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cls([p], lr=0.1)
    # an instance that got a CPU parameter some other way refuses at the step, and nothing moves
    opt = optim.convert(torch.optim.AdamW([p], lr=0.1))
    assert isinstance(opt, torch.optim.AdamW) and isinstance(opt, optim._HipStep)
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(5)) and len(opt.state) == 0


def test_classes_are_torch_classes():
    assert issubclass(optim.HipAdamW, torch.optim.AdamW) and issubclass(optim.HipAdam, torch.optim.Adam)
    assert optim.hip_step_class(torch.optim.AdamW) is optim.HipAdamW and optim.hip_step_class(torch.optim.Adam) is optim.HipAdam
