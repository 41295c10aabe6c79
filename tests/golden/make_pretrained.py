#!/usr/bin/env python
"""Generate tests/golden/pretrained.json by running the REFERENCE's own ``get_model`` (imported from /root/reference, like
make_golden.py) on the synthetic checkpoints of tests/pretrained_case.py: per case the state_dict's key / shape / dtype order, the
trainable parameters (sha256 digests) and a sha256 per sub-model whose values came from a file; plus the key contract of the
full R101 dec6 model.
``--check``: regenerate in memory and compare with the committed file (exit status 1 on a difference).

The reference downloads what it lacks; here nothing may reach a URL:
  * torchvision (absent) is tests/golden/_tv_standin.py; its resnetN factories are wrapped so that ``pretrained=True`` does what
    torchvision 0.7 does with a cached file -- a strict load of ``<hub dir>/checkpoints/<file>``;
  * the reference's resnet_multiimage_input keeps running its own tiling code: its ``model_zoo`` is a local loader whose
    "URLs" (``model_urls``) are the cached file names;
  * MachineConfig.DOWNLOAD_MODEL_DIR points at the temporary directory and download_model_if_doesnt_exist only asserts that
    the checkpoint is there.
"""
import json
import os
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "pretrained.json")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import _tv_standin  # noqa: E402
import pretrained_case as PC  # noqa: E402

_tv_standin.install()
sys.path.insert(0, REF)
_loader = types.ModuleType("loader")
_loader.__path__ = [os.path.join(REF, "loader")]
sys.modules["loader"] = _loader

_tv = sys.modules["torchvision.models"]
_resnet = sys.modules["torchvision.models.resnet"]


def _local(name):
    return torch.load(os.path.join(torch.hub.get_dir(), "checkpoints", name), map_location="cpu")


def _pretrained_factory(make, n):
    def factory(pretrained=False, **kw):
        model = make(False, **kw)
        if pretrained:
            model.load_state_dict(_local(PC.IMNET_FILES[n]), strict=True)
        return model
    return factory


for _n in (18, 34, 50, 101, 152):
    setattr(_tv, "resnet%d" % _n, _pretrained_factory(getattr(_tv, "resnet%d" % _n), _n))
_resnet.model_urls = {"resnet%d" % n: f for n, f in PC.IMNET_FILES.items()}

from configs.machine_config import MachineConfig  # noqa: E402
import models.resnet_encoder as ref_resnet_encoder  # noqa: E402
import models.utils as ref_utils  # noqa: E402
from models import get_model as ref_get_model  # noqa: E402

ref_resnet_encoder.model_zoo = types.SimpleNamespace(load_url=_local)
ref_resnet_encoder.models = _tv


def _exists_only(model_name, download_dir=None):
    path = os.path.join(MachineConfig.DOWNLOAD_MODEL_DIR, model_name, "depth.pth")
    assert os.path.isfile(path), path


ref_utils.download_model_if_doesnt_exist = _exists_only


def generate():
    tmp = tempfile.mkdtemp(prefix="segsde_pretrained_")
    hub, models_dir = os.path.join(tmp, "hub"), os.path.join(tmp, "models")
    torch.hub.set_dir(hub)
    MachineConfig.DOWNLOAD_MODEL_DIR = models_dir
    PC.write_all(hub, models_dir)
    out = {"cases": {}}
    for name, (cfg, prefixes) in sorted(PC.cases().items()):
        torch.manual_seed(0)
        rec = PC.record(ref_get_model(json.loads(json.dumps(cfg)), PC.N_CLASSES), prefixes)
        rec["cfg"] = PC.cfg_digest(cfg)
        out["cases"][name] = rec
        print(name, rec["n_keys"], "entries")
    PC.write_imnet(hub, 101, const=True)
    m = ref_get_model(PC.dec6_r101_cfg(), PC.N_CLASSES)
    out["dec6_r101"] = dict(PC.contract(m), cfg=PC.cfg_digest(PC.dec6_r101_cfg()))
    print("dec6_r101", out["dec6_r101"]["n_keys"], "entries")
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    data = generate()
    if "--check" in sys.argv:
        with open(OUT) as f:
            same = json.load(f) == data
        print("pretrained.json matches" if same else "pretrained.json DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
