#!/usr/bin/env python
"""tests/golden/berhu.npz: inputs, loss and gradient of the BerHu pseudo-depth loss as the REFERENCE computes them -- its own
``loss/loss.py::berhu`` (imported from /root/reference; build container only), fp32 on the CPU, the gradient from autograd.  Numbers
only: four cases of [2,1,10,16] tensors (plain, apply_log, the own-car mask of train.py:491-494, a general 0/1 mask), inputs uniform
in (0, 1) from np.random.RandomState.  tests/berhu_cases.py pins its float64 oracle to these.

    python tests/golden/make_berhu.py            # write the fixture
    python tests/golden/make_berhu.py --check    # regenerate and compare with the committed file, bit for bit
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "berhu.npz")
sys.dont_write_bytecode = True
SHAPE = (2, 1, 10, 16)
CASES = (("plain", False, "none", 101), ("log", True, "none", 102), ("own_car", False, "own_car", 103), ("mask", False, "general", 104))


def _reference():
    path = os.path.join(REF, "loss", "loss.py")
    spec = importlib.util.spec_from_file_location("reference_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.realpath(mod.__file__).startswith(REF)
    return mod


def build():
    ref = _reference()
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, apply_log, kind, seed in CASES:
        r = np.random.RandomState(seed)
        x = (1e-3 + 0.998 * r.uniform(size=SHAPE)).astype(np.float32)
        t = (1e-3 + 0.998 * r.uniform(size=SHAPE)).astype(np.float32)
        if kind == "own_car":
            m = np.ones(SHAPE, dtype=np.float32)
            m[:, :, int(SHAPE[2] * 0.9):, :] = 0
        elif kind == "general":
            m = (r.uniform(size=SHAPE) < 0.7).astype(np.float32)
        else:
            m = np.ones(SHAPE, dtype=np.float32)
        xi = torch.from_numpy(x).clone().requires_grad_(True)
        loss = ref.berhu(xi, torch.from_numpy(t), torch.from_numpy(m), apply_log=apply_log)
        loss.backward()
        assert loss.dtype == torch.float32 and xi.grad.dtype == torch.float32 and bool(torch.isfinite(xi.grad).all())
        out[name + "_x"], out[name + "_t"], out[name + "_m"] = x, t, m
        out[name + "_apply_log"] = np.array(apply_log)
        out[name + "_loss"] = loss.detach().numpy().copy()
        out[name + "_grad"] = xi.grad.numpy().copy()
    return out


def main():
    new = build()
    if "--check" in sys.argv:
        old = np.load(OUT, allow_pickle=False)
        assert sorted(old.files) == sorted(new)
        for k in new:
            assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k
        print("berhu.npz matches")
        return
    np.savez_compressed(OUT, **new)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
