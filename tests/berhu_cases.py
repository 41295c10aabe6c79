"""BerHu pseudo-depth loss (hipops.berhu_forward / berhu_backward, csrc/berhu.hip, loss.loss.berhu / berhu_own_car, the two callers
in trainer.py): the cases shared by the interpreter run (test_berhu_emu.py) and the GPU run (test_berhu_gpu.py).

The oracle is a float64 numpy restatement of the formula (value and gradient, C from its own maximum, sign(0) = 0); it is pinned to
the reference by tests/golden/berhu.npz (written by tests/golden/make_berhu.py from the reference's loss/loss.py).  Nothing is
compared against the code under test.

Tolerances (the package's 3 x rule): on the same inputs the reference formula is evaluated in fp32 with torch on the CPU; its error
against the oracle is the yardstick.  The HIP result may err at most 3 x as much, with one floor: 4 eps32 |oracle| for the loss (all
terms are non-negative and accumulated in double; each carries at most three fp32 roundings and the result one more) and
4 eps32 max|oracle gradient| for the gradient's maximum error.
Exact, not tolerances: without apply_log state[0] is the fp32 maximum of |t - x| * m bit for bit and state[1] is
float32(0.2 * float64(state[0])); the gradient is exactly 0.0 at every masked, cropped or t == x element; two runs return identical
bits; the own-car crop equals the materialised-mask call bit for bit."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import berhu, berhu_own_car

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
THRESHOLD = 0.2

# csrc/berhu.hip launches min(768, ceil(n / 1024)) blocks of 256 threads (3 per compute unit of the MI355X), each thread one quad of
# four elements per trip: a trip of the grid-stride loop covers 768 * 1024 = 786 432 elements.  BIG (880 102 elements, <= 2^20)
# takes a second, partly filled trip; it is no multiple of 4, so it has a scalar tail as well.
GRID_BLOCKS = 768
BIG = (2, 1, 431, 1021)
assert GRID_BLOCKS * 1024 < int(np.prod(BIG)) <= 2 ** 20 and int(np.prod(BIG)) % 4 != 0

SHAPES = [(1, 1, 1, 1), (2, 1, 5, 7), (3, 1, 33, 65), (2, 1, 64, 128), BIG]
# mode -> (apply_log, mask kind)
MODES = {"plain": (False, "none"), "log": (True, "none"), "own_car": (False, "own_car"), "own_car_log": (True, "own_car"),
         "mask": (False, "general"), "mask_log": (True, "general"), "row_mask": (False, "rows")}
GENERATED = [(11 + i, s, m) for i, s in enumerate(SHAPES[:4]) for m in ("plain", "log", "own_car", "mask")] + \
            [(21, (3, 1, 33, 65), "own_car_log"), (22, (2, 1, 64, 128), "mask_log"), (23, (3, 1, 33, 65), "row_mask"),
             (24, (2, 1, 10, 16), "row_mask"), (31, BIG, "plain"), (32, BIG, "own_car_log")]


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def keep_rows_of(shape, keep=0.9):
    return int(shape[-2] * keep)


def own_car_mask(shape, keep=0.9):
    """the tensor both callers of the reference build (train.py:491-494, 871-874)"""
    m = np.ones(shape, dtype=F32)
    m[..., keep_rows_of(shape, keep):, :] = 0
    return m


# ------------------------------------------------------------------------------------------------------------------ oracle
def oracle(x, t, m=None, apply_log=False, g=1.0):
    """float64: -> (loss, d loss / d x times g [shape of the broadcast], info).  C = 0.2 max(a) is a constant for the gradient;
    sign(0) = 0; max(a) = 0 gives loss 0 and a zero gradient."""
    x64, t64 = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    m64 = np.ones((), dtype=np.float64) if m is None else np.asarray(m, dtype=np.float64)
    x64, t64, m64 = np.broadcast_arrays(x64, t64, m64)
    xl, tl = (np.log(1.0 + x64), np.log(1.0 + t64)) if apply_log else (x64, t64)
    d = tl - xl
    a = np.abs(d) * m64
    C = THRESHOLD * float(a.max())
    lin = a <= C
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(lin, a, (a * a + C * C) / (2.0 * C))
        fac = np.where(lin, 1.0, a / C)
    grad = g / a.size * -np.sign(d) * m64 * fac
    if apply_log:
        grad = grad / (1.0 + x64)
    return float(val.mean()), grad, {"max": float(a.max()), "C": C, "lin": lin, "a": a, "d": d}


def reference_f32(x, t, m=None, apply_log=False):
    """the reference's formula (loss.py:5-15) in fp32 with torch on the CPU, autograd for the gradient: the yardstick"""
    xi = torch.from_numpy(np.ascontiguousarray(x)).clone().requires_grad_(True)
    ti = torch.from_numpy(np.ascontiguousarray(t))
    mi = torch.ones((), dtype=torch.float32) if m is None else torch.from_numpy(np.ascontiguousarray(m))
    a, b = (torch.log(1 + xi), torch.log(1 + ti)) if apply_log else (xi, ti)
    absdiff = torch.abs(b - a) * mi
    C = THRESHOLD * torch.max(absdiff).item()
    loss = torch.mean(torch.where(absdiff <= C, absdiff, (absdiff * absdiff + C * C) / (2 * C)))
    loss.backward()
    return float(loss.detach()), xi.grad.numpy().astype(np.float64)


def gate_loss(got, want, ref, what):
    e, e_ref, floor = abs(float(got) - want), abs(ref - want), 4.0 * EPS32 * abs(want)
    print("%-46s loss: oracle %.9g | e_ref %.3e | e_hip %.3e | ratio %.2f | floor %.3e" % (
        what, want, e_ref, e, e / e_ref if e_ref > 0 else float("inf") if e > 0 else 0.0, floor))
    assert np.isfinite(got) and e <= max(3.0 * e_ref, floor), "%s: loss error %.3e > max(3 x %.3e, %.3e)" % (what, e, e_ref, floor)


def gate_grad(got, want, ref, what):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), what + ": non-finite gradient"
    # max(a) == 0 (everything masked, or t == x): the reference's gradient is NaN, no yardstick -- then only the floor is left
    e, e_ref = float(np.abs(got - want).max()), float(np.abs(ref - want).max()) if np.all(np.isfinite(ref)) else 0.0
    floor = 4.0 * EPS32 * float(np.abs(want).max())
    print("%-46s grad: max|oracle| %.3e | e_ref %.3e | e_hip %.3e | ratio %.2f | floor %.3e" % (
        what, np.abs(want).max(), e_ref, e, e / e_ref if e_ref > 0 else float("inf") if e > 0 else 0.0, floor))
    assert e <= max(3.0 * e_ref, floor), "%s: gradient error %.3e > max(3 x %.3e, %.3e)" % (what, e, e_ref, floor)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).reshape(-1).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ inputs
def generate(seed, shape, mode):
    """x, t uniform in (0, 1); mask by kind: none, the own-car tensor, a general 0/1 tensor of the full shape, or [B,1,H,1] rows.
    -> dict(x, t, m (what the call gets, or None), m_full (what the oracle gets), keep_rows, apply_log)"""
    apply_log, kind = MODES[mode]
    r = np.random.RandomState(seed)
    x = (1e-3 + 0.998 * r.uniform(size=shape)).astype(F32)
    t = (1e-3 + 0.998 * r.uniform(size=shape)).astype(F32)
    m = m_full = keep_rows = None
    if kind == "own_car":
        keep_rows, m_full = keep_rows_of(shape), own_car_mask(shape)
    elif kind == "general":
        m = m_full = (r.uniform(size=shape) < 0.7).astype(F32)
    elif kind == "rows":
        m = (r.uniform(size=(shape[0], 1, shape[2], 1)) < 0.7).astype(F32)
        if m.size > 1:
            m.reshape(-1)[0], m.reshape(-1)[-1] = 1, 0            # both values occur
        m_full = np.broadcast_to(m, shape)
    return {"x": x, "t": t, "m": m, "m_full": m_full, "keep_rows": keep_rows, "apply_log": apply_log}


@functools.lru_cache(maxsize=None)
def generated(seed, shape, mode):
    """the inputs, the oracle and the yardstick of one case: computed once, shared by the tests, never modified"""
    c = generate(seed, shape, mode)
    want = oracle(c["x"], c["t"], c["m_full"], c["apply_log"])
    ref = reference_f32(c["x"], c["t"], c["m_full"], c["apply_log"])
    info = want[2]
    n = c["x"].size
    live = np.ones(shape, bool) if c["m_full"] is None else (c["m_full"] != 0)
    if n >= 64:      # both branches of the loss are populated
        frac = float((info["lin"] & live).sum()) / float(live.sum())
        assert 0.1 <= frac <= 0.9, "seed %d %s %s: %.3f of the unmasked elements in the linear branch" % (seed, shape, mode, frac)
    assert_sign_is_decided(info["d"][live], c["apply_log"], "seed %d %s %s" % (seed, shape, mode))
    return c, want, ref


def assert_sign_is_decided(d, apply_log, what):
    """t - x of two fp32 numbers has its exact sign in fp32; log(1 + t) - log(1 + x) carries up to three roundings of values below
    0.7 (4 eps32 is well above them): no live element may sit where they decide the sign -- the gradient would jump by 2 g / n"""
    if apply_log:
        assert not np.any((d != 0) & (np.abs(d) < 4 * EPS32)), what + ": a log difference below 4 eps32, choose another seed"


def dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run_ops(device, c, x=None, t=None, m=None, g=1.0, keep_rows="case"):
    """hipops forward + backward on the case's (or the given) device tensors -> (loss [1], state [2], grad) as numpy"""
    x = dev(c["x"], device) if x is None else x
    t = dev(c["t"], device) if t is None else t
    m = dev(c["m"], device) if m is None else m
    kr = c["keep_rows"] if keep_rows == "case" else keep_rows
    loss, state = H.berhu_forward(x, t, m, kr, c["apply_log"])
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (1,) and tuple(state.shape) == (2,)
    assert loss.device.type == torch.device(device).type
    gs = torch.full((1,), g, dtype=torch.float32, device=device)
    dx = H.berhu_backward(x, t, state, gs, m, kr, c["apply_log"])
    assert dx.dtype == torch.float32 and tuple(dx.shape) == tuple(c["x"].shape)
    return loss.cpu().numpy(), state.cpu().numpy(), dx.cpu().numpy()


def check_exact_state(state, c, what):
    """without apply_log: the kernel and this check take a maximum over identical fp32 values"""
    m = F32(1) if c["m_full"] is None else c["m_full"]
    want_max = (np.abs(c["t"] - c["x"]) * m).astype(F32).max()
    assert bits(state[0])[0] == bits(want_max)[0], "%s: max %r != %r" % (what, state[0], want_max)
    want_C = F32(THRESHOLD * np.float64(state[0]))
    assert bits(state[1])[0] == bits(want_C)[0], "%s: C %r != %r" % (what, state[1], want_C)


def check_zero_grad(dx, c, info, what):
    dead = info["a"] == 0                                   # masked, cropped, t == x
    assert np.all(dx[dead] == 0.0), what + ": a gradient at a masked / cropped / t == x element"
    assert np.all(dx[~dead] != 0.0), what + ": a zero gradient at a live element"


def run_generated(device, seed, shape, mode):
    c, (want_loss, want_grad, info), (ref_loss, ref_grad) = generated(seed, shape, mode)
    what = "seed %d %s %s" % (seed, case_id(shape), mode)
    loss, state, dx = run_ops(device, c)
    gate_loss(loss[0], want_loss, ref_loss, what)
    gate_grad(dx, want_grad, ref_grad, what)
    if not c["apply_log"]:
        check_exact_state(state, c, what)
    else:
        assert abs(float(state[0]) - info["max"]) <= 8 * EPS32 * info["max"] and abs(float(state[1]) - info["C"]) <= 8 * EPS32 * info["C"]
    check_zero_grad(dx, c, info, what)
    again = run_ops(device, c)
    for a, b, name in zip((loss, state, dx), again, ("loss", "state", "grad")):
        assert np.array_equal(bits(a), bits(b)), "%s: two runs differ in %s" % (what, name)
    if c["keep_rows"] is not None:                          # the crop from the element index == the materialised mask
        mat = run_ops(device, c, m=dev(c["m_full"], device), keep_rows=None)
        for a, b, name in zip((loss, state, dx), mat, ("loss", "state", "grad")):
            assert np.array_equal(bits(a), bits(b)), "%s: crop and mask tensor differ in %s" % (what, name)


# ------------------------------------------------------------------------------------------------------------------ layouts
def run_misaligned(device):
    """tensors that start 4 and 8 bytes into their storage: the base pointers are not 16-byte aligned (element-wise path), alone
    and mixed with aligned operands; same bits as the aligned call"""
    c, (want_loss, want_grad, info), (ref_loss, ref_grad) = generated(13, (3, 1, 33, 65), "mask")

    def shifted(a, k):
        flat = torch.zeros(a.size + k, dtype=torch.float32, device=device)
        flat[k:] = dev(a, device).reshape(-1)
        v = flat[k:].view(a.shape)
        assert v.data_ptr() % 16 == (4 * k) % 16 and v.is_contiguous()
        return v

    base = run_ops(device, c)
    for what, kx, kt, km in (("all off by 4 bytes", 1, 1, 1), ("off by 4 / 8 / 12", 1, 2, 3), ("only the target", 0, 1, 0),
                             ("only the mask", 0, 0, 2)):
        got = run_ops(device, c, x=shifted(c["x"], kx), t=shifted(c["t"], kt), m=shifted(c["m"], km))
        gate_loss(got[0][0], want_loss, ref_loss, "misaligned, " + what)
        gate_grad(got[2], want_grad, ref_grad, "misaligned, " + what)
        check_exact_state(got[1], c, what)
        check_zero_grad(got[2], c, info, what)
        assert np.array_equal(bits(got[1]), bits(base[1])) and np.array_equal(bits(got[2]), bits(base[2])), what


def run_broadcast_mask(device):
    """a [B,1,H,1] mask against [B,1,H,W] operands, and an input broadcast against a larger target through the autograd Function"""
    for seed, shape in ((23, (3, 1, 33, 65)), (24, (2, 1, 10, 16))):
        run_generated(device, seed, shape, "row_mask")
    c, _, _ = generated(24, (2, 1, 10, 16), "row_mask")
    x = dev(c["x"][:, :, :, :1], device).requires_grad_(True)          # [B,1,H,1] against the [B,1,H,W] target
    berhu(x, dev(c["t"], device), dev(c["m"], device)).backward()
    col = np.ascontiguousarray(c["x"][:, :, :, :1])
    want = oracle(col, c["t"], c["m_full"])[1].sum(-1, keepdims=True)
    assert tuple(x.grad.shape) == tuple(x.shape)
    gate_grad(x.grad.cpu().numpy(), want, reference_f32(col, c["t"], c["m_full"])[1], "broadcast input")


# ------------------------------------------------------------------------------------------------------------------ planted
def run_last_element_maximum(device):
    """a difference of 5.0 in the last element of the tensor -- in the scalar tail of the 16-byte path (n % 4 != 0), and the last
    element of the element-wise path -- sets C"""
    for seed, shape, shift in ((41, (2, 1, 5, 7), 0), (42, (3, 1, 33, 65), 0), (43, (3, 1, 33, 65), 1), (44, (2, 1, 64, 128), 0)):
        c = generate(seed, shape, "plain")
        c["t"].reshape(-1)[-1] = c["x"].reshape(-1)[-1] + F32(5.0)
        want_loss, want_grad, info = oracle(c["x"], c["t"])
        ref_loss, ref_grad = reference_f32(c["x"], c["t"])
        assert info["max"] > 4.9 and int(info["a"].reshape(-1).argmax()) == c["x"].size - 1
        x, t = dev(c["x"], device), dev(c["t"], device)
        if shift:
            fx, ft = torch.zeros(x.numel() + 1, device=device), torch.zeros(x.numel() + 1, device=device)
            fx[1:], ft[1:] = x.reshape(-1), t.reshape(-1)
            x, t = fx[1:].view(shape), ft[1:].view(shape)
        what = "last-element maximum %s%s" % (case_id(shape), " (misaligned)" if shift else "")
        loss, state, dx = run_ops(device, c, x=x, t=t)
        check_exact_state(state, c, what)
        assert abs(float(state[1]) - 1.0) < 1e-5, (what, state)
        gate_loss(loss[0], want_loss, ref_loss, what)
        gate_grad(dx, want_grad, ref_grad, what)


def run_maximum_inside_crop(device):
    """a difference of 5.0 inside the cropped rows must not set C; the crop equals the materialised mask bit for bit, and
    berhu_own_car equals berhu with the reference's keep tensor"""
    for seed, shape in ((51, (2, 1, 10, 16)), (52, (2, 1, 33, 65)), (53, (1, 1, 10, 7))):
        for apply_log in (False, True):
            c = generate(seed, shape, "own_car_log" if apply_log else "own_car")
            kr = c["keep_rows"]
            assert kr == int(0.9 * shape[2]) and kr < shape[2]
            for b, row, col in ((0, kr, 0), (shape[0] - 1, shape[2] - 1, shape[3] - 1)):
                c["t"][b, 0, row, col] = c["x"][b, 0, row, col] + F32(5.0)
            want_loss, want_grad, info = oracle(c["x"], c["t"], c["m_full"], apply_log)
            ref_loss, ref_grad = reference_f32(c["x"], c["t"], c["m_full"], apply_log)
            assert info["max"] < 1.0
            what = "maximum inside the crop %s%s" % (case_id(shape), " log" if apply_log else "")
            loss, state, dx = run_ops(device, c)
            assert float(state[0]) < 1.0, (what, state)
            if not apply_log:
                check_exact_state(state, c, what)
            gate_loss(loss[0], want_loss, ref_loss, what)
            gate_grad(dx, want_grad, ref_grad, what)
            check_zero_grad(dx, c, info, what)
            mat = run_ops(device, c, m=dev(c["m_full"], device), keep_rows=None)
            for a, b_, name in zip((loss, state, dx), mat, ("loss", "state", "grad")):
                assert np.array_equal(bits(a), bits(b_)), "%s: crop and mask tensor differ in %s" % (what, name)
            # the public functions: berhu_own_car against berhu with the keep tensor the reference builds
            xa, xb = dev(c["x"], device).requires_grad_(True), dev(c["x"], device).requires_grad_(True)
            t = dev(c["t"], device)
            keep = torch.ones(shape, device=device)
            keep[:, :, int(shape[2] * 0.9):, :] = 0
            la, lb = berhu_own_car(xa, t, apply_log=apply_log), berhu(xb, t, keep, apply_log=apply_log)
            la.backward()
            lb.backward()
            assert la.dim() == 0 and torch.equal(la.detach(), lb.detach()) and torch.equal(xa.grad, xb.grad), what
            assert np.array_equal(bits(la.detach().cpu().numpy()), bits(loss)), what


def run_equal_inputs(device):
    """x == t everywhere: loss 0.0, an all-zero gradient, no NaN (the reference's gradient is NaN here: documented deviation)"""
    for shape in ((1, 1, 1, 1), (2, 1, 5, 7), (2, 1, 33, 65)):
        for mode in ("plain", "log", "own_car", "mask"):
            c = generate(61, shape, mode)
            c["t"] = c["x"].copy()
            loss, state, dx = run_ops(device, c)
            assert loss[0] == 0.0 and state[0] == 0.0 and state[1] == 0.0, (shape, mode, loss, state)
            assert np.all(dx == 0.0), (shape, mode)
            x = dev(c["x"], device).requires_grad_(True)
            m = dev(c["m_full"], device) if c["m_full"] is not None else torch.ones(shape, device=device)
            l = berhu(x, dev(c["t"], device), m, apply_log=c["apply_log"])
            l.backward()
            assert float(l.detach()) == 0.0 and bool((x.grad == 0).all())


# ------------------------------------------------------------------------------------------------------------------ autograd
def run_autograd_retain_graph(device):
    """x = sigmoid(p); berhu(x, t, m).backward(retain_graph=True); then a second loss through the same x: the reference's call
    sequence (train.py:489-510).  p.grad against the oracle's chain, evaluated at the x the device produced."""
    shape = (2, 1, 33, 65)
    for apply_log in (False, True):
        r = np.random.RandomState(71)
        p0 = r.normal(0.0, 1.5, shape).astype(F32)
        c = generate(72, shape, "mask_log" if apply_log else "mask")
        w = r.normal(0.0, 1.0, shape).astype(F32)
        p = dev(p0, device).requires_grad_(True)
        x = torch.sigmoid(p)
        t, m, wd = dev(c["t"], device), dev(c["m"], device), dev(w, device)
        first = berhu(x, t, m, apply_log=apply_log)
        assert first.dim() == 0 and first.dtype == torch.float32
        first.backward(retain_graph=True)
        g_first = p.grad.detach().clone()
        second = (x * wd).mean()
        second.backward()
        xv = x.detach().cpu().numpy()
        x64 = xv.astype(np.float64)
        want_loss, gx, info = oracle(xv, c["t"], c["m_full"], apply_log)
        assert_sign_is_decided(info["d"][c["m_full"] != 0], apply_log, "autograd case")
        chain = x64 * (1.0 - x64)
        want = (gx + w.astype(np.float64) / w.size) * chain
        ref_loss, rgx = reference_f32(xv, c["t"], c["m_full"], apply_log)
        ref = ((rgx.astype(F32) + w / F32(w.size)) * (xv * (F32(1) - xv))).astype(np.float64)
        what = "retain_graph then a second backward%s" % (" log" if apply_log else "")
        gate_loss(float(first.detach()), want_loss, ref_loss, what)
        gate_grad(g_first.cpu().numpy(), gx * chain, (rgx.astype(F32) * (xv * (F32(1) - xv))).astype(np.float64), what + ", first")
        gate_grad(p.grad.cpu().numpy(), want, ref, what + ", both")


def run_scaled_backward(device):
    """a GradScaler-style backward: the loss times 2^16 gives exactly 2^16 times the gradient"""
    for seed, shape, mode in ((13, (3, 1, 33, 65), "mask"), (21, (3, 1, 33, 65), "own_car_log")):
        c, _, _ = generated(seed, shape, mode)
        grads = []
        for scale in (1.0, 65536.0):
            x = dev(c["x"], device).requires_grad_(True)
            t = dev(c["t"], device)
            loss = berhu_own_car(x, t, apply_log=c["apply_log"]) if c["keep_rows"] is not None else \
                berhu(x, t, dev(c["m"], device), apply_log=c["apply_log"])
            (loss * scale).backward()
            grads.append(x.grad.detach().cpu())
        assert bool((grads[0] != 0).any()) and torch.equal(grads[1], grads[0] * 65536.0), mode


def run_requires_grad_refused(device):
    import pytest
    c, _, _ = generated(12, (2, 1, 5, 7), "mask")
    x, t, m = dev(c["x"], device), dev(c["t"], device), dev(c["m"], device)
    with pytest.raises(NotImplementedError):
        berhu(x.clone().requires_grad_(True), t.clone().requires_grad_(True), m)
    with pytest.raises(NotImplementedError):
        berhu(x, t, m.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        berhu_own_car(x, t.clone().requires_grad_(True))
    with torch.no_grad():                                   # nothing is differentiated: fine
        berhu(x, t.clone().requires_grad_(True), m)


def run_python_argument_checks(device="cpu"):
    """refused in Python, before the library is looked up"""
    import pytest
    z = torch.zeros(2, 1, 4, 6, device=device)
    with pytest.raises(TypeError):
        H.berhu_forward(z, z.long())
    with pytest.raises(TypeError):
        H.berhu_forward(z, z, mask=z > 0)
    with pytest.raises(RuntimeError):
        H.berhu_forward(z, torch.zeros(2, 1, 4, 5, device=device))       # not broadcastable
    with pytest.raises(ValueError):
        H.berhu_forward(z[:0], z[:0])
    for kr in (-1, 5):
        with pytest.raises(ValueError):
            H.berhu_forward(z, z, keep_rows=kr)
    with pytest.raises(ValueError):
        H.berhu_forward(z.reshape(-1), z.reshape(-1), keep_rows=1)
    with pytest.raises(ValueError):
        H.berhu_backward(z, z, torch.zeros(3, device=device), torch.ones(1, device=device))
    with pytest.raises(ValueError):
        H.berhu_backward(z, z, torch.zeros(2, device=device), torch.ones(2, device=device))


def run_torch_op(device):
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    assert "segsde::berhu" in TO.names() and hasattr(torch.ops.segsde, "berhu")
    c, _, _ = generated(13, (3, 1, 33, 65), "mask")
    x, t, m = dev(c["x"], device), dev(c["t"], device), dev(c["m"], device)
    a = torch.ops.segsde.berhu(x, t, m)
    assert a.dim() == 0 and torch.equal(a, berhu(x, t, m))
    b = torch.ops.segsde.berhu(x, t, None, keep_rows_of(x.shape), True)
    assert torch.equal(b, berhu_own_car(x, t, apply_log=True))
    xg = x.clone().requires_grad_(True)
    torch.ops.segsde.berhu(xg, t, m).backward()
    xh = x.clone().requires_grad_(True)
    berhu(xh, t, m).backward()
    assert torch.equal(xg.grad, xh.grad)


def run_profile_kind(device, monkeypatch):
    """both directions go through hipops._timed under the hbm_berhu kind"""
    seen = []
    real = H._timed
    monkeypatch.setattr(H, "_timed", lambda kind, *a, **k: (seen.append(kind), real(kind, *a, **k))[1])
    c, _, _ = generated(12, (2, 1, 5, 7), "mask")
    run_ops(device, c)
    assert seen == ["hbm_berhu", "hbm_berhu"]


# ------------------------------------------------------------------------------------------------------------------ the fixture
def run_oracle_vs_fixture():
    """tests/golden/berhu.npz: inputs, the reference's fp32 loss and its autograd gradient (CPU) for four cases.  An fp32 result
    against a float64 one, a few roundings per element: rtol 1e-6 for the loss, 1e-6 of the gradient's maximum magnitude."""
    z = np.load(os.path.join(GOLDEN, "berhu.npz"), allow_pickle=False)
    names = [str(n) for n in z["cases"]]
    assert names == ["plain", "log", "own_car", "mask"]
    for n in names:
        x, t, m = z[n + "_x"], z[n + "_t"], z[n + "_m"]
        assert x.dtype == F32 and t.dtype == F32 and m.dtype == F32
        apply_log = bool(z[n + "_apply_log"])
        loss, grad, info = oracle(x, t, m, apply_log)
        assert abs(loss - float(z[n + "_loss"])) <= 1e-6 * abs(loss), (n, loss, float(z[n + "_loss"]))
        assert np.abs(grad - z[n + "_grad"]).max() <= 1e-6 * np.abs(grad).max(), n
        frac = info["lin"][m != 0].mean()
        assert 0.1 <= frac <= 0.9, (n, frac)
        if n == "own_car":
            assert np.array_equal(m, own_car_mask(m.shape))
        # and the yardstick of these tests is that very formula
        rl, rg = reference_f32(x, t, m, apply_log)
        assert abs(rl - float(z[n + "_loss"])) <= 4 * EPS32 * abs(loss)
        assert np.abs(rg - z[n + "_grad"]).max() <= 4 * EPS32 * np.abs(grad).max()


def fixture_cases():
    z = np.load(os.path.join(GOLDEN, "berhu.npz"), allow_pickle=False)
    return [(str(n), z[str(n) + "_x"], z[str(n) + "_t"], z[str(n) + "_m"], bool(z[str(n) + "_apply_log"]), float(z[str(n) + "_loss"]),
             z[str(n) + "_grad"]) for n in z["cases"]]


def run_fixture_on_device(device):
    """the kernels on the fixture's inputs, against the oracle with the recorded reference numbers as the yardstick"""
    for n, x, t, m, apply_log, ref_loss, ref_grad in fixture_cases():
        c = {"x": x, "t": t, "m": m, "m_full": m, "keep_rows": None, "apply_log": apply_log}
        want_loss, want_grad, info = oracle(x, t, m, apply_log)
        loss, state, dx = run_ops(device, c)
        gate_loss(loss[0], want_loss, ref_loss, "fixture " + n)
        gate_grad(dx, want_grad, ref_grad.astype(np.float64), "fixture " + n)
        if n == "own_car":
            c2 = dict(c, m=None, keep_rows=keep_rows_of(x.shape))
            got = run_ops(device, c2)
            assert np.array_equal(bits(got[0]), bits(loss)) and np.array_equal(bits(got[2]), bits(dx))


# ------------------------------------------------------------------------------------------------------------------ callers
class _DispStub(torch.nn.Module):
    """the part of the model's interface trainer.validate uses with segmentation off and pose disabled: a dict in, a dict with
    ("disp", 0) out, parameters, the training flag, predict_test_disp; a fixed 1x1 convolution and a sigmoid in plain torch"""

    def __init__(self):
        super().__init__()
        self.head = torch.nn.Conv2d(3, 1, 1)
        with torch.no_grad():
            g = torch.Generator().manual_seed(81)
            self.head.weight.copy_(3.0 * torch.randn(1, 3, 1, 1, generator=g))
            self.head.bias.copy_(torch.randn(1, generator=g))

    def forward(self, inputs):
        return {("disp", 0): torch.sigmoid(self.head(inputs[("color_aug", 0, 0)]))}

    def predict_test_disp(self, inputs):
        return {}


class _NoMono:
    def generate_depth_test_pred(self, outputs):
        pass


def run_validate(device):
    """trainer.validate with cfg["data"]["depth_teacher"] set: two batches of (2,1,10,16) disparities, pseudo_depth_loss_log on and
    off; losses["pseudo_depth_loss"] = the mean of the oracle's per-batch values; the returned keys are unchanged"""
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    model = _DispStub().to(device)
    r = np.random.RandomState(82)
    batches = [{("color_aug", 0, 0): dev(r.uniform(size=(2, 3, 10, 16)).astype(F32), device),
                "pseudo_depth": dev((1e-3 + 0.998 * r.uniform(size=(2, 1, 10, 16))).astype(F32), device)} for _ in range(2)]
    for use_log in (True, False):
        cfg = {"model": {"disable_monodepth": False, "disable_pose": True}, "data": {"depth_teacher": "mono_cityscapes"},
               "training": {"amp": False, "segmentation_lambda": 0.0, "monodepth_lambda": 1.0, "n_tensorboard_imgs": 0,
                            "pseudo_depth_loss_log": use_log}}
        want, ref = [], []
        model.eval()
        for b in batches:
            with torch.no_grad():
                disp = model(dict(b))[("disp", 0)].cpu().numpy()
            assert disp.shape == (2, 1, 10, 16)
            pd = b["pseudo_depth"].cpu().numpy()
            o = oracle(disp, pd, own_car_mask(disp.shape), use_log)
            assert 0.1 <= o[2]["lin"][own_car_mask(disp.shape) != 0].mean() <= 0.9
            want.append(o[0])
            ref.append(reference_f32(disp, pd, own_car_mask(disp.shape), use_log)[0])
        model.train()
        out = T.validate(model, [dict(b) for b in batches], cfg, 19, monodepth_loss_calculator_val=_NoMono())
        assert model.training
        assert set(out) == {"losses", "score", "class_iou", "depth", "imgs_to_save"}
        assert set(out["losses"]) == {"segmentation_loss", "monodepth_loss", "pseudo_depth_loss"}
        assert out["losses"]["segmentation_loss"] == 0.0 and out["losses"]["monodepth_loss"] == 0.0
        got = out["losses"]["pseudo_depth_loss"]
        assert isinstance(got, float)
        gate_loss(got, float(np.mean(want)), float(np.mean(np.asarray(ref, dtype=F32), dtype=np.float64)),
                  "validate, pseudo_depth_loss_log %s" % use_log)
    # without a depth_teacher the term stays the integer zero
    cfg0 = dict(cfg, data={})
    out = T.validate(model, [dict(b) for b in batches], cfg0, 19, monodepth_loss_calculator_val=_NoMono())
    assert out["losses"]["pseudo_depth_loss"] == 0.0


def run_train_step(device):
    """trainer.train_step on the tiny ResNet-18 contract configuration at 32 x 64 with pseudo_depth_lambda = 1, monodepth_lambda = 0,
    segmentation_lambda = 1: pseudo_depth_loss equals the oracle on the disparity of an identical copy of the model (same mode,
    dropout off), and the depth decoder receives gradients"""
    import trainstep_case as TC
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import cross_entropy2d
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    cfg = TC.full_cfg("joint")
    cfg["training"].update(pseudo_depth_lambda=1.0, monodepth_lambda=0.0, segmentation_lambda=1.0)
    sd = TC.state_dict("joint")

    def make():
        m = get_model(cfg["model"], TC.NCLS)
        m.load_state_dict(sd, strict=True)
        TC.no_dropout(m)
        return m.to(device)

    inputs = {k: v.to(device) for k, v in TC.batch(100).items()}
    r = np.random.RandomState(91)
    pd = (1e-3 + 0.998 * r.uniform(size=(TC.B, 1, TC.HH, TC.WW))).astype(F32)
    inputs["pseudo_depth"] = dev(pd, device)
    twin = make()
    twin.train()
    with torch.no_grad():
        disp = twin(dict(inputs))[("disp", 0)].float().cpu().numpy()
    assert disp.shape == pd.shape
    mask = own_car_mask(disp.shape)
    want, _, info = oracle(disp, pd, mask)
    ref, _ = reference_f32(disp, pd, mask)
    model = make()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    losses = T.train_step(model, opt, dict(inputs), 0, cfg, lambda input, target: cross_entropy2d(input, target), None)
    got = float(losses["pseudo_depth_loss"])
    assert np.isfinite(got) and got > 0.0
    assert losses["pseudo_depth_loss"].dim() == 0 and losses["pseudo_depth_loss"].device.type == torch.device(device).type
    gate_loss(got, want, ref, "train_step pseudo_depth_loss")
    assert float(losses["mono_loss"]) == 0.0 and float(losses["segmentation_loss"]) > 0.0
    total = float(losses["segmentation_total_loss"]) + got
    assert abs(float(losses["total_loss"]) - total) <= 1e-6 * total
    depth = [(k, p) for k, p in model.named_parameters() if k.startswith("models.depth.")]
    assert depth, sorted({k.split(".")[1] for k, _ in model.named_parameters()})
    # only ("disp", 0) feeds a loss: the disparity heads of the three coarser scales (two parameters each, among decoder.14-17)
    # stay without a gradient, every other parameter of the depth decoder gets a finite one that is not all zero
    heads = ("models.depth.decoder.14.", "models.depth.decoder.15.", "models.depth.decoder.16.", "models.depth.decoder.17.")
    dead = [k for k, p in depth if p.grad is None or not bool((p.grad != 0).any())]
    assert len(dead) <= 6 and all(k.startswith(heads) for k in dead), dead
    assert all(bool(torch.isfinite(p.grad).all()) for _, p in depth if p.grad is not None)
    assert len(depth) - len(dead) >= 24, (len(depth), dead)


# ------------------------------------------------------------------------------------------------------------------ GPU only
def run_no_sync(device):
    """forward and backward of berhu and of berhu_own_car with torch's synchronisation debug mode set to "error", after a warm-up
    call (the first call loads the library)"""
    import pytest
    c, _, _ = generated(13, (3, 1, 33, 65), "mask")
    x0, t, m = dev(c["x"], device), dev(c["t"], device), dev(c["m"], device)

    def both():
        out = []
        for f in (lambda x: berhu(x, t, m), lambda x: berhu_own_car(x, t, apply_log=True)):
            x = x0.clone().requires_grad_(True)
            loss = f(x)
            loss.backward()
            out.append((loss.detach(), x.grad))
        return out

    warm = both()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        try:
            torch.cuda.set_sync_debug_mode("error")
        except Exception as e:                              # noqa: BLE001
            pytest.skip("this torch build has no synchronisation debug mode on ROCm: %s" % e)
        got = both()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for (la, ga), (lb, gb) in zip(warm, got):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
