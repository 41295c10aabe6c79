"""Synthetic pretrained checkpoints and the model configurations that load them, shared by tests/golden/make_pretrained.py (the
reference's ``get_model`` on these files -> tests/golden/pretrained.json), tests/test_pretrained.py (the package on the kernel
interpreter) and tests/test_pretrained_gpu.py.

Values come from numpy's seeded RandomState, one stream per key (a function of the seed and the key name only), so the files -- and
the hashes of what loads them -- are the same on every machine.  The files are laid out as the reference expects them:
* ImageNet: ``<hub dir>/checkpoints/resnetN-xxxxxxxx.pth`` -- torchvision 0.7's keys, ``fc.*`` included, no num_batches_tracked
  (like the published files);
* ``mono_*``: ``<model dir>/<name>/{encoder,depth,pose_encoder,pose}.pth`` -- what save_monodepth_models writes; encoder.pth here
  also carries the height / width / use_stereo ints of a monodepth2 checkpoint and lacks one key (MISSING_KEY)."""
import copy
import hashlib
import json
import os
import zlib

import numpy as np
import torch

SEED = 20240
N_CLASSES = 19
MONO = "mono_synthetic_r18"                  # the mono_* checkpoint directory of the R18 cases
MISSING_KEY = "encoder.layer4.1.bn2.bias"     # absent from encoder.pth: keeps its initial value (0) under strict=False
IMNET_FILES = {18: "resnet18-5c106cde.pth", 34: "resnet34-333f7ec4.pth", 50: "resnet50-19c8e357.pth",
               101: "resnet101-5d3b4d8f.pth", 152: "resnet152-b121ed2f.pth"}


def _value(key, shape, dtype, seed, const=False):
    if dtype == torch.int64:
        return torch.tensor(7, dtype=torch.int64) if len(shape) == 0 else torch.full(shape, 7, dtype=torch.int64)
    if const:
        return torch.full(shape, 0.5, dtype=torch.float32)
    rs = np.random.RandomState((seed + zlib.crc32(key.encode())) % (2 ** 32))
    n = rs.standard_normal(shape).astype(np.float32)
    leaf = key.rsplit(".", 1)[-1]
    if leaf == "running_var":
        v = 0.75 + 0.5 * rs.random_sample(shape).astype(np.float32)
    elif leaf == "running_mean":
        v = 0.1 * n
    elif leaf == "weight" and len(shape) == 1:         # BatchNorm gamma
        v = 1.0 + 0.1 * n
    elif leaf == "bias":
        v = 0.05 * n
    else:                                              # conv / linear weights: unit gain over the fan-in
        v = n * np.float32(1.0 / np.sqrt(max(1, int(np.prod(shape[1:])))))
    return torch.from_numpy(np.ascontiguousarray(v.astype(np.float32)))


def fill(spec, seed=SEED, const=False):
    """spec: [(key, shape, dtype)] -> state_dict with the seeded values (const: a constant, for key / shape contracts)"""
    return {k: _value(k, tuple(s), d, seed, const) for k, s, d in spec}


def spec_of(module):
    return [(k, tuple(v.shape), v.dtype) for k, v in module.state_dict().items()]


def imnet_spec(num_layers):
    """torchvision 0.7's ResNet state_dict keys of an ImageNet checkpoint: the package's ResNet (same names) without
    num_batches_tracked, plus the classifier"""
    from improving_segmentation_with_selfsupervised_depth_amd.models.resnet_encoder import ResNet, _SPECS
    block, layers = _SPECS[num_layers]
    spec = [s for s in spec_of(ResNet(block, layers)) if not s[0].endswith("num_batches_tracked")]
    return spec + [("fc.weight", (1000, 512 * block.expansion), torch.float32), ("fc.bias", (1000,), torch.float32)]


def write_imnet(hub_dir, num_layers, const=False):
    d = os.path.join(hub_dir, "checkpoints")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, IMNET_FILES[num_layers])
    torch.save(fill(imnet_spec(num_layers), SEED + num_layers, const), path)
    return path


def base_cfg(backbone="resnet18", rswd=None, height=64, width=128, **kw):
    """a monodepth model of the dec6 family (intermediate ASPP decoder, three frames, pose pairs) at a small size"""
    cfg = dict(arch="joint_segmentation_depth", backbone_name=backbone, replace_stride_with_dilation=rswd,
               segmentation_name=None, segmentation_args=None, pose_model_input="pairs", provide_uncropped_for_pose=False,
               backbone_pretraining="none", depth_pretraining="none", pose_pretraining="none", freeze_backbone=False,
               freeze_depth=False, freeze_pose=False, freeze_segmentation=True, disable_monodepth=False, disable_pose=False,
               enable_imnet_encoder=False, frame_ids=[0, -1, 1], num_scales=4, height=height, width=width,
               depth_args=dict(intermediate_aspp=True, aspp_rates=[6, 12, 18], n_upconv=4, num_ch_dec=[64, 128, 128, 256, 256],
                               max_scale_size=[height, width]))
    cfg.update(kw)
    return cfg


def cases():
    """name -> (model cfg, state_dict key prefixes whose values come from the files)"""
    jsd_args = dict(weights="none", layers=[9], head_inter_channels=64, layer_out_channels=64, head_dropout=0.1, layer_dropout=0,
                    head_inter=False, output_stride=1)
    return {
        # (a) R18 joint model, ImageNet backbone -> the 6-channel pose encoder gets ImageNet R18 weights too
        "a_imnet_joint": (base_cfg(segmentation_name="joint_seg_depth_dec", segmentation_args=jsd_args, freeze_segmentation=False,
                                   backbone_pretraining="imnet"),
                          ["models.encoder.", "models.pose_encoder."]),
        # (b) mono_* backbone, depth and pose
        "b_mono_all": (base_cfg(backbone_pretraining=MONO, depth_pretraining=MONO, pose_pretraining=MONO),
                       ["models.encoder.", "models.depth.", "models.pose_encoder.", "models.pose."]),
        # (c) dec6-style: ImageNet backbone + frozen ImageNet encoder, mono_* depth and pose
        "c_dec6": (base_cfg(backbone_pretraining="imnet", depth_pretraining=MONO, pose_pretraining=MONO, enable_imnet_encoder=True),
                   ["models.encoder.", "models.imnet_encoder.", "models.depth.", "models.pose_encoder.", "models.pose."]),
    }


def dec6_r101_cfg():
    """the model block of configs/cityscapes_monodepth_highres_dec6.yml (R101, dilated layer4, ImageNet encoder) with its mono_*
    depth / pose initialisation left out (key / shape / order contract only)"""
    cfg = base_cfg("resnet101", [False, False, True], 512, 1024, backbone_pretraining="imnet", enable_imnet_encoder=True)
    cfg["depth_args"]["max_scale_size"] = [512, 1024]
    return cfg


def mono_files(cfg, model_dir, name=MONO, seed=SEED + 1000, const=False):
    """write <model_dir>/<name>/{encoder,depth,pose_encoder,pose}.pth for a model of ``cfg``'s architecture"""
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    plain = copy.deepcopy(cfg)
    plain.update(backbone_pretraining="none", depth_pretraining="none", pose_pretraining="none", enable_imnet_encoder=False)
    m = get_model(plain, N_CLASSES).cpu()
    d = os.path.join(model_dir, name)
    os.makedirs(d, exist_ok=True)
    for mn in ("encoder", "depth", "pose_encoder", "pose"):
        sd = fill(spec_of(m.models[mn]), seed + zlib.crc32(mn.encode()) % 1000, const)
        if mn == "encoder":
            sd = {k: v for k, v in sd.items() if k != MISSING_KEY}
            sd.update(height=512, width=1024, use_stereo=False)
        torch.save(sd, os.path.join(d, mn + ".pth"))
    return d


def write_all(hub_dir, model_dir, layers=(18,)):
    for n in layers:
        write_imnet(hub_dir, n)
    mono_files(cases()["b_mono_all"][0], model_dir)


def _sha(items):
    h = hashlib.sha256()
    for it in items:
        h.update((it if isinstance(it, bytes) else json.dumps(it).encode()) + b"\0")
    return h.hexdigest()


def cfg_digest(cfg):
    return _sha([json.loads(json.dumps(cfg, sort_keys=True))])


def contract(model):
    """sha256 digests of the state_dict's key / shape / dtype order and of the trainable parameter names, with the entry count"""
    sd = model.state_dict()
    return {"n_keys": len(sd),
            "keys": _sha([[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]),
            "trainable": _sha([k for k, p in model.named_parameters() if p.requires_grad])}


def record(model, prefixes):
    """what the fixture stores of a built model: its contract and, per sub-model whose values come from files, one sha256 over
    its keys and values in order (loading is a copy or an exact cat-and-divide, so these match bit for bit)"""
    sd = model.state_dict()
    rec = contract(model)
    rec["values"] = {p: _sha(b for k, v in sd.items() if k.startswith(p)
                             for b in (k.encode(), np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()))
                     for p in prefixes}
    return rec
