"""CPU: the BerHu pseudo-depth loss (hipops.berhu_forward / berhu_backward, csrc/berhu.hip, loss.loss.berhu / berhu_own_car and their
callers in trainer.py) with the kernels run by the interpreter build of the real sources -- the cases of berhu_cases.py against its
float64 oracle -- plus what needs no kernel at all: the oracle against the reference's recorded numbers, the prototypes in header
and binding, argument validation in Python and of the hipcc-built library, the operator registration."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import berhu_cases as C
import emu
from conftest import REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

NEW = ["segsde_berhu_workspace", "segsde_berhu_forward", "segsde_berhu_backward"]


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_oracle_matches_reference_fixture():
    C.run_oracle_vs_fixture()


@pytest.mark.parametrize("seed,shape,mode", C.GENERATED, ids=C.case_id)
def test_generated(interp, seed, shape, mode):
    """fails without the feature: hipops.berhu_forward does not exist"""
    C.run_generated("cpu", seed, shape, mode)


def test_fixture_inputs(interp):
    C.run_fixture_on_device("cpu")


def test_misaligned_base_pointers(interp):
    C.run_misaligned("cpu")


def test_broadcast_mask(interp):
    C.run_broadcast_mask("cpu")


def test_last_element_maximum(interp):
    C.run_last_element_maximum("cpu")


def test_maximum_inside_crop(interp):
    C.run_maximum_inside_crop("cpu")


def test_equal_inputs(interp):
    C.run_equal_inputs("cpu")


def test_autograd_retain_graph(interp):
    C.run_autograd_retain_graph("cpu")


def test_scaled_backward(interp):
    C.run_scaled_backward("cpu")


def test_requires_grad_refused(interp):
    C.run_requires_grad_refused("cpu")


def test_torch_op(interp):
    C.run_torch_op("cpu")


def test_profile_kind(interp, monkeypatch):
    C.run_profile_kind("cpu", monkeypatch)


def test_validate(interp):
    C.run_validate("cpu")


def test_train_step(interp):
    C.run_train_step("cpu")


def test_python_argument_checks():
    C.run_python_argument_checks("cpu")


def test_signatures():
    from improving_segmentation_with_selfsupervised_depth_amd.loss import loss as L
    assert str(inspect.signature(L.berhu)) == "(input, target, mask, apply_log=False)"
    assert str(inspect.signature(L.berhu_own_car)) == "(input, target, apply_log=False, keep=0.9)"
    assert ".item()" not in inspect.getsource(L.berhu) + inspect.getsource(L.berhu_own_car) + inspect.getsource(L._berhu) + \
        inspect.getsource(L._BerHuFn)


def test_callers_allocate_no_mask():
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    for fn in (T.train_step, T.validate):
        src = inspect.getsource(fn)
        assert "berhu_own_car(" in src and "torch.ones(" not in src, fn.__name__


def test_torch_op_registered():
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    assert "segsde::berhu" in TO.names()
    assert torch.ops.segsde.berhu is not None


def test_new_prototypes_in_header_and_binding():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS
    assert int(re.search(r"#define SEGSDE_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 26


def test_argument_validation_without_gpu():
    """the codes of include/segsde_hip.h, returned before any launch by the hipcc-built library"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    L = _lib.bind(ctypes.CDLL(ge.LIB))
    assert L.segsde_abi_version() == _lib.ABI_VERSION == 26
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    fwd = lambda **k: L.segsde_berhu_forward(*[k.get(n, d) for n, d in (      # noqa: E731
        ("x", fake), ("t", fake), ("m", None), ("n", 640), ("H", 10), ("W", 16), ("keep", 9), ("log", 0), ("thr", 0.2), ("loss", fake),
        ("state", fake), ("ws", fake), ("ws_bytes", 1 << 20), ("stream", None))])
    bwd = lambda **k: L.segsde_berhu_backward(*[k.get(n, d) for n, d in (     # noqa: E731
        ("x", fake), ("t", fake), ("m", None), ("n", 640), ("H", 10), ("W", 16), ("keep", 9), ("log", 0), ("state", fake), ("g", fake),
        ("dx", fake), ("stream", None))])
    assert fwd(x=None) == -1 and fwd(t=None) == -1 and fwd(loss=None) == -1 and fwd(state=None) == -1 and fwd(ws=None) == -1
    assert bwd(x=None) == -1 and bwd(t=None) == -1 and bwd(state=None) == -1 and bwd(g=None) == -1 and bwd(dx=None) == -1
    for call in (fwd, bwd):
        assert call(n=0) == -2 and call(n=-4) == -2
        assert call(keep=-2) == -2 and call(keep=11) == -2                      # 0 <= keep_rows <= H
        assert call(n=641) == -2 and call(H=0) == -2 and call(W=0) == -2        # H * W divides n
        assert call(x=odd) == -4 and call(t=odd) == -4 and call(m=odd) == -4
    assert fwd(thr=0.0) == -2 and fwd(thr=-1.0) == -2 and fwd(thr=float("nan")) == -2 and fwd(thr=float("inf")) == -2
    need = L.segsde_berhu_workspace(640)
    assert need > 0 and fwd(ws_bytes=need - 1) == -3 and fwd(ws_bytes=0) == -3
    assert L.segsde_berhu_workspace(0) == 0 and L.segsde_berhu_workspace(-1) == 0
    assert L.segsde_berhu_workspace(1 << 40) == L.segsde_berhu_workspace(1 << 30) >= need      # the grid is capped
    assert fwd(ws=ctypes.c_void_p(4100)) == -4 and fwd(loss=odd) == -4 and bwd(dx=odd) == -4
