"""CPU: the batched mix masks (csrc/mixmask.hip: the "depthhist" histogram thresholds, the batched "depth" and ClassMix masks;
hipops, loader.transformmasks, trainer.generate_mix_mask) with the kernels run by the interpreter build of the real sources -- the
cases of mix_mask_cases.py against np.histogram and against the per-image formulation of the parent commit -- plus what needs no
kernel: prototypes in header and binding, argument validation of the hipcc-built library and in Python."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import emu
import mix_mask_cases as C
from conftest import REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

NEW = ["segsde_depth_hist_workspace", "segsde_depth_hist_thresholds", "segsde_depth_threshold_mask_batch", "segsde_class_presence",
       "segsde_class_mask_batch"]


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("gen,shape,seed", C.HIST_CASES, ids=C.case_id)
def test_histogram_bit_for_bit(interp, gen, shape, seed):
    """fails without the feature: hipops.depth_hist_thresholds does not exist"""
    C.run_hist_case("cpu", gen, shape, seed)


@pytest.mark.parametrize("gen,shape,seed", C.FALLBACK_CASES, ids=C.case_id)
def test_stale_max_depth(interp, gen, shape, seed):
    C.run_fallback_behind_uniform("cpu", gen, shape, seed)


@pytest.mark.parametrize("B", C.BATCHES)
def test_fused_log_and_public_function(interp, B):
    """fails without the feature: "depthhist" raises NotImplementedError"""
    C.run_fused_log("cpu", B)


@pytest.mark.parametrize("B", C.BATCHES)
def test_class_identity(interp, B):
    C.run_class_identity("cpu", B)


def test_class_id_range(interp):
    C.run_class_id_range("cpu")


@pytest.mark.parametrize("B,shape", [(1, (8, 16)), (2, (33, 67)), (5, (33, 67)), (2, (64, 128))], ids=C.case_id)
def test_depth_identity(interp, B, shape):
    C.run_depth_identity("cpu", B, shape)


def test_untouched_modes(interp):
    C.run_untouched_modes("cpu")


def test_python_argument_checks(interp):
    C.run_python_argument_checks("cpu")


def test_cpu_tensor_refused(monkeypatch):
    """a CPU tensor handed to the real library raises instead of computing anywhere else"""
    import __graft_entry__ as ge
    from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
    if not os.path.exists(ge.LIB):
        ge.build()
    monkeypatch.setattr(_lib, "_LIB", _lib.bind(ctypes.CDLL(ge.LIB)))
    monkeypatch.setattr(_lib, "HOST_POINTERS_OK", False)
    d, pred = torch.rand(2, 1, 8, 16), torch.zeros(2, 8, 16, dtype=torch.int64)
    for call in (lambda: H.depth_hist_thresholds(d, torch.rand(2)), lambda: H.depth_threshold_mask_batch(d, torch.rand(2)),
                 lambda: H.class_presence(pred), lambda: H.class_mask_batch(pred, torch.zeros(2, 256, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_no_unique_in_generate_mix_mask():
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    from improving_segmentation_with_selfsupervised_depth_amd.loader import transformmasks as TM
    src = inspect.getsource(T.generate_mix_mask)
    assert "torch.unique" not in src and "not part of the path" not in src and '"depthhist"' in src
    assert "torch.unique" not in inspect.getsource(TM.generate_class_mix_masks)
    assert str(inspect.signature(T.generate_mix_mask)) == \
        "(mode, argmax_u_w, unlabeled_imgs, depths, depthcomp_margin=0.03, depthcomp_foreground_threshold=0.0)"


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
    fake, odd2, odd4 = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(4100)

    def caller(fn, spec):
        return lambda **k: fn(*[k.get(n, d) for n, d in spec])

    hist = caller(L.segsde_depth_hist_thresholds, (("d", fake), ("B", 2), ("HW", 640), ("log", 1), ("u", fake), ("table", fake),
                                                   ("counts", None), ("ws", fake), ("ws_bytes", 1 << 20), ("stream", None)))
    thr = caller(L.segsde_depth_threshold_mask_batch, (("d", fake), ("B", 2), ("HW", 640), ("thr", fake), ("stride", 1), ("mask", fake),
                                                       ("stream", None)))
    pres = caller(L.segsde_class_presence, (("pred", fake), ("B", 2), ("HW", 640), ("counts", fake), ("stream", None)))
    cmask = caller(L.segsde_class_mask_batch, (("pred", fake), ("B", 2), ("HW", 640), ("sel", fake), ("mask", fake), ("stream", None)))
    assert hist(d=None) == -1 and hist(u=None) == -1 and hist(table=None) == -1 and hist(ws=None) == -1
    assert thr(d=None) == -1 and thr(thr=None) == -1 and thr(mask=None) == -1
    assert pres(pred=None) == -1 and pres(counts=None) == -1
    assert cmask(pred=None) == -1 and cmask(sel=None) == -1 and cmask(mask=None) == -1
    for call in (hist, thr, pres, cmask):
        assert call(B=0) == -2 and call(B=-1) == -2 and call(HW=0) == -2 and call(HW=-5) == -2 and call(HW=1 << 31) == -2
        assert call(B=65536) == -4
    assert thr(stride=-1) == -2
    need = L.segsde_depth_hist_workspace(2, 640)
    assert need >= 2 * (2 * 4 + 2 * 4 + 100 * 4)
    assert hist(ws_bytes=need - 1) == -3 and hist(ws_bytes=0) == -3
    assert L.segsde_depth_hist_workspace(0, 640) == 0 and L.segsde_depth_hist_workspace(2, 0) == 0
    assert L.segsde_depth_hist_workspace(2, 1 << 31) == 0
    assert L.segsde_depth_hist_workspace(16, 512 * 1024) > L.segsde_depth_hist_workspace(16, 640)
    # null before shape before workspace before alignment
    assert hist(d=None, B=0) == -1 and hist(B=0, ws_bytes=0) == -2 and hist(d=odd2, ws_bytes=0) == -3
    assert hist(d=odd2) == -4 and hist(u=odd2) == -4 and hist(table=odd2) == -4 and hist(counts=odd2) == -4 and hist(ws=odd2) == -4
    assert thr(d=odd2) == -4 and thr(thr=odd2) == -4 and thr(mask=odd2) == -4
    assert pres(pred=odd4) == -4 and pres(counts=odd2) == -4
    assert cmask(pred=odd4) == -4 and cmask(mask=odd4) == -4
