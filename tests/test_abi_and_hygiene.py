"""CPU: the C-ABI header, the ctypes binding and the built libraries agree symbol-for-symbol; the product package
never touches the oracle or a CPU fallback; ops fail loudly without the extension / without a GPU tensor."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

PKG = os.path.join(REPO, "improving_segmentation_with_selfsupervised_depth_amd")


def header_symbols():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(segsde_[a-z0-9_]+)\s*\(", txt)))


def test_header_matches_binding():
    assert header_symbols() == _lib.EXPORTS


def test_real_library_exports_every_symbol():
    """hipcc-built libsegsde_hip.so (built by __graft_entry__.build(); no kernel is launched here)"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    cdll = ctypes.CDLL(ge.LIB)
    for name in header_symbols():
        assert hasattr(cdll, name), name
    assert cdll.segsde_abi_version() == _lib.ABI_VERSION
    # the code objects inside are gfx950
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o", "--input=" + ge.LIB],
                         capture_output=True, text=True).stdout
    if out.strip():
        assert "gfx950" in out


def test_argument_validation_without_gpu():
    """bad descriptors are rejected before any launch (safe to call without a GPU)"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    cdll = _lib.bind(ctypes.CDLL(ge.LIB))
    d = _lib.ConvDesc()
    assert cdll.segsde_conv2d_forward(ctypes.byref(d), None, None, None, None, None, None, None) == -2
    d = _lib.ConvDesc(B=1, H=4, W=4, C0=4, C1=0, ld0=4, Ho=4, Wo=4, Cout=4, ldy=4, KH=3, KW=3, stride=1, dil=1, pad=1)
    assert cdll.segsde_conv2d_forward(ctypes.byref(d), None, None, None, None, None, None, None) == -1
    assert cdll.segsde_conv2d_wgrad_workspace(ctypes.byref(d)) > 0
    assert cdll.segsde_bn_stats(None, 4, 10, 4, None, None, None, None, 0.1, 1e-5, None, None, 0, None) == -1
    # round-5 entries: the one-kernel Winograd weight gradient / data-gradient, the border kernel, dropout, the geometry adjoints
    dw = _lib.ConvDesc(B=2, H=8, W=16, C0=64, C1=0, ld0=64, Ho=8, Wo=16, Cout=64, ldy=64, KH=3, KW=3, stride=1, dil=1, pad=1)
    assert cdll.segsde_conv2d_wgrad_winograd_fused_workspace(ctypes.byref(dw)) > 0
    dw.KH = dw.KW = 1
    dw.pad = 0
    assert cdll.segsde_conv2d_wgrad_winograd_fused_workspace(ctypes.byref(dw)) == 0          # not a 3x3: the caller takes another route
    assert cdll.segsde_conv2d_wgrad_winograd_fused(ctypes.byref(dw), None, None, None, 64, None, None, 0, None) == -1
    fake = ctypes.c_void_p(4096)
    assert cdll.segsde_conv2d_wgrad_winograd_fused(ctypes.byref(dw), fake, None, fake, 64, fake, fake, 1 << 30, None) == -4
    assert cdll.segsde_conv2d_winograd_fused_dgrad(None, 64, 2, 8, 16, 64, None, 64, 64, None, 64, 0, None, 0, 0, None) == -1
    assert cdll.segsde_conv2d_winograd_fused_dgrad(fake, 64, 2, 7, 16, 64, fake, 64, 64, fake, 64, 0, None, 0, 0, None) == -4   # odd height
    assert cdll.segsde_conv2d_winograd_fused_dgrad(fake, 64, 2, 8, 16, 64, fake, 32, 64, fake, 64, 0, None, 0, 0, None) == -4   # pack narrower than its slice
    assert cdll.segsde_conv2d_winograd_fused2(fake, 64, 48, 1, fake, 64, 16, 2, 8, 16, 1, fake, 64, None, 0, fake, 64, None, None) == -4  # C0 % 64
    # the one-kernel forward addresses one image of a source with 32-bit byte offsets: 2048 x 2048 pixels at a pitch of 256 floats is 4 GiB
    assert cdll.segsde_conv2d_winograd_fused(fake, 256, 1, 2048, 2048, 64, 0, fake, 64, None, 0, fake, 64, 0, None, None) == -4
    assert cdll.segsde_conv2d_winograd_fused_dgrad(fake, 256, 1, 2048, 2048, 64, fake, 64, 64, fake, 64, 0, None, 0, 0, None) == -4
    assert cdll.segsde_conv2d_winograd_fused2(fake, 64, 64, 0, fake, 256, 64, 1, 2048, 2048, 1, fake, 64, None, 0, fake, 64, None, None) == -4
    assert cdll.segsde_winograd_fused_pack(fake, 64, 32, 1, fake, None) == -4             # N = 32: no partial block in the pack layout
    assert cdll.segsde_reflect_adjoint_borders2(None, 64, None, 64, None, 64, None, 0, 0, 2, 8, 16, 64, 64, None) == -1
    assert cdll.segsde_reflect_adjoint_borders2(fake, 64, fake, 64, fake, 64, None, 0, 0, 2, 3, 16, 64, 64, None) == -4         # H < 4
    assert cdll.segsde_dropout(None, 4, 10, 4, 0.5, 1, None, 4, None) == -1
    assert cdll.segsde_dropout(fake, 4, 10, 4, 1.0, 1, fake, 4, None) == -2
    assert cdll.segsde_project3d_backward_workspace(0, 8, 8) == 0 and cdll.segsde_project3d_backward_workspace(2, 8, 8) > 0
    assert cdll.segsde_project3d_backward(fake, fake, fake, fake, 2, 8, 8, 1e-7, None, fake, None, 0, None) == -3               # d T needs the workspace
    assert cdll.segsde_backproject_depth_backward(None, None, 2, 8, 8, None, None) == -1
    # the smoothness adjoint checks its shape like the forward (w == 1 would divide by zero in its normalisation)
    assert cdll.segsde_smoothness_forward(fake, fake, 2, 8, 1, fake, fake, fake, 1 << 20, None) == -2
    assert cdll.segsde_smoothness_backward(fake, fake, fake, 2, 8, 1, 1.0, fake, fake, 1 << 20, None) == -2
    assert cdll.segsde_smoothness_backward(fake, fake, fake, 0, 8, 8, 1.0, fake, fake, 1 << 20, None) == -2
    assert cdll.segsde_smoothness_backward(fake, fake, fake, 2, 1, 8, 1.0, fake, fake, 1 << 20, None) == -2


def pointer_lifetime_violations(path):
    """(line, text) of every place in a Python source where an address is taken of a tensor no name holds: the argument of
    ``_p(...)`` / ``H._p(...)`` and the receiver of ``.data_ptr()`` may contain no call other than ``_f32(<name or attribute>)``
    (which returns its argument).  ``_p(t.contiguous())`` is the defect this guards against: for a strided ``t`` the copy is
    released when ``_p`` returns, before the kernel is launched.  Subscripts (views of a held buffer) are fine."""
    import ast
    src = open(path).read()
    tree = ast.parse(src, path)

    def plain(n):
        return isinstance(n, ast.Name) or (isinstance(n, ast.Attribute) and plain(n.value))

    def allowed(call):
        f = call.func
        is_f32 = (isinstance(f, ast.Name) and f.id == "_f32") or (isinstance(f, ast.Attribute) and f.attr == "_f32" and plain(f.value))
        return is_f32 and len(call.args) >= 1 and plain(call.args[0]) and not call.keywords and \
            all(isinstance(a, ast.Constant) for a in call.args[1:])

    def temporaries(expr):
        if isinstance(expr, ast.Subscript):                  # a view of what ``value`` holds; the index may compute what it likes
            return temporaries(expr.value)
        mine = [expr] if isinstance(expr, ast.Call) and not allowed(expr) else []
        return mine + [c for child in ast.iter_child_nodes(expr) for c in temporaries(child)]

    bad = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if (isinstance(f, ast.Name) and f.id == "_p") or (isinstance(f, ast.Attribute) and f.attr == "_p"):
            exprs = list(node.args)
        elif isinstance(f, ast.Attribute) and f.attr == "data_ptr":
            exprs = [f.value]
        else:
            continue
        if any(temporaries(e) for e in exprs):
            bad.append((node.lineno, ast.get_source_segment(src, node)))
    return bad


def package_sources():
    return sorted(os.path.join(root, f) for root, _, files in os.walk(PKG) for f in files if f.endswith(".py"))


def test_no_pointer_of_a_temporary():
    """every tensor whose address goes to a kernel is held by a name of the caller (hipops' "Operand lifetime" note)"""
    bad = {os.path.relpath(p, REPO): v for p in package_sources() for v in [pointer_lifetime_violations(p)] if v}
    assert not bad, bad
    # the textual form of the same defect
    pat = re.compile(r"_p\((_f32\()?[^()]*\.(contiguous|float|to)\(")
    hits = [(os.path.relpath(p, REPO), i + 1) for p in package_sources() for i, line in enumerate(open(p)) if pat.search(line)]
    assert not hits, hits


def test_pointer_guard_sees_the_defect(tmp_path):
    """the guard flags the forms it exists for and passes the held ones"""
    f = tmp_path / "sample.py"
    f.write_text("def a(t):\n    return _p(_f32(t.contiguous()))\n"
                 "def b(t):\n    return H._p(t.contiguous())\n"
                 "def c(tables):\n    return tables.nearest(1, 2).data_ptr()\n"
                 "def d(t, buf):\n    t = t.contiguous()\n    return _p(_f32(t)), _p(buf[1:]), H._p(H._f32(t)), buf[0].data_ptr(), _p(_f32(t, 'x'))\n")
    assert [ln for ln, _ in pointer_lifetime_violations(str(f))] == [2, 4, 6]


def test_product_never_imports_oracle_or_falls_back():
    bad = []
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "hipemu" in src or "libsegsde_emu" in src:
                    bad.append(os.path.join(root, f))
    assert not bad, bad


def test_ops_fail_loudly(monkeypatch, tmp_path):
    from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
    # (1) missing shared object
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "HOST_POINTERS_OK", False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_cpu_tensor_rejected(monkeypatch):
    """a CPU tensor handed to an op of the real library raises instead of computing anywhere else"""
    import __graft_entry__ as ge
    from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
    if not os.path.exists(ge.LIB):
        ge.build()
    monkeypatch.setattr(_lib, "_LIB", _lib.bind(ctypes.CDLL(ge.LIB)))
    monkeypatch.setattr(_lib, "HOST_POINTERS_OK", False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.colsum(torch.zeros(4, 4))


def test_launch_bracketing_samples_every_site_once(monkeypatch):
    """bench.py's kernel timing (hipops._timed, PROFILE_PERIOD): launch q of step i is bracketed iff (q + i) % P == 0 -- over P
    steps every launch site is timed exactly once, every launch is recorded (population), and the executed-FLOP figure of the
    dilated windows follows the kernels' tile-uniform dead-row rule"""
    import torch
    from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

    class Ev:
        def __init__(self, enable_timing=True):
            pass

        def record(self, stream=None):
            pass

    class Like:
        is_cuda = True

    monkeypatch.setattr(torch.cuda, "Event", Ev)
    monkeypatch.setattr(H, "PROFILE", [])
    monkeypatch.setattr(H, "PROFILE_PERIOD", 5)
    ran = []
    for i in range(5):
        H.profile_step(i)
        for q in range(7):
            H._timed("conv_fwd", 1.0, Like(), lambda: ran.append(1), "site%d" % q)
    assert len(ran) == 35 and len(H.PROFILE) == 35
    timed = sorted(r[4] for r in H.PROFILE if r[2] is not None)
    assert timed == ["site%d" % q for q in range(7)]
    # live share of the ASPP windows on the 32 x 64 bottleneck map
    for dil, want in ((6, 0.875), (12, 0.75), (18, 0.625)):
        g = H.ConvGeom(2048, 256, 3, 1, dil, dil, False, 0, False)
        assert abs(H._live_tap_frac(g, 32, 64) - want) < 1e-9 and abs(H._live_tap_frac(g, 32, 64, wgrad=True) - want) < 1e-9
    assert H._live_tap_frac(H.ConvGeom(256, 256, 3, 1, 1, 1, False, 0, False), 32, 64) == 1.0


def test_signatures_match_reference():
    """tests/golden/signatures.json = ``inspect.signature`` of every constructor / function / method of the drop-in boundary as
    the reference defines it (tests/golden/make_signatures.py imports /root/reference).  The package's object must take the
    same parameters, in the same order, with the same defaults; it may add trailing parameters only if they have defaults
    (``skip`` / ``up`` of the decoder blocks, test hooks of the augmentations) -- every reference call site keeps working."""
    import importlib
    import inspect
    import json
    from conftest import GOLDEN
    ref = json.load(open(os.path.join(GOLDEN, "signatures.json")))
    assert len(ref) >= 50
    extras, bad = {}, []
    for key, want in sorted(ref.items()):
        mod, name = key.split(":")
        obj = importlib.import_module("improving_segmentation_with_selfsupervised_depth_amd." + mod)
        try:
            for part in name.split("."):
                obj = getattr(obj, part)
        except AttributeError:
            bad.append((key, "missing"))
            continue
        got = inspect.signature(obj)
        if str(got) == want:
            continue
        # same leading parameters (name, kind, default), extras defaulted
        wp = want.strip()[1:-1]
        gp = list(got.parameters.values())
        n_ref = len(inspect.signature(eval("lambda " + wp.replace("self", "self_") + ": 0")).parameters) if wp else 0
        lead = str(inspect.Signature(gp[:n_ref]))
        rest = gp[n_ref:]
        if lead.replace("self_", "self") != want or any(p.default is inspect.Parameter.empty and p.kind not in
                                                           (p.VAR_KEYWORD, p.VAR_POSITIONAL) for p in rest):
            bad.append((key, want, str(got)))
        else:
            extras[key] = [p.name for p in rest]
    assert not bad, bad
    print("wider than the reference:", extras)
    # the only places where the package's signature is wider than the reference's
    assert set(extras) <= {"models.monodepth_layers:ConvBlock.forward", "models.monodepth_layers:Conv3x3.forward",
                           "loader.transformsgpu:color_jitter", "loader.transformsgpu:gaussian_blur",
                           "models.model_parts:ASPP.forward", "models.model_parts:SelfAttention.forward"}, extras
