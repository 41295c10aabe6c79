"""Mirror of models/utils.py builders (get_resnet_backbone, get_depth_decoder, get_posenet, _get_layer).

Pretrained initialisation reads local files only -- the reference downloads what it lacks (Google Drive, torchvision's model zoo),
this package never does; a missing file is a FileNotFoundError naming the path looked for:

* ``mono_*`` checkpoints (backbone / depth / pose): ``<DOWNLOAD_MODEL_DIR>/<name>/{encoder,depth,pose_encoder,pose}.pth``, the files
  the reference unpacks from its downloads and ``trainer.save_monodepth_models`` writes.  ``DOWNLOAD_MODEL_DIR`` is
  this module's attribute, set by the caller; left at None it is ``configs.machine_config.MachineConfig.DOWNLOAD_MODEL_DIR`` when
  that module is importable (under the reference's train.py it is).
* ImageNet weights (``"imnet"``): torchvision's cached file, see resnet_encoder.imnet_checkpoint_path."""
import errno
import os
import re

import torch
from torch import nn

from .depth_decoder import DepthDecoder
from .pose_decoder import PoseDecoder
from .resnet_encoder import ResnetEncoder


DOWNLOAD_MODEL_DIR = None      # directory of the mono_* checkpoints; see the module docstring


def _device():
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def model_dir():
    """the directory the reference's MachineConfig.DOWNLOAD_MODEL_DIR names (models/utils.py:27,51,80)"""
    if DOWNLOAD_MODEL_DIR is not None:
        return DOWNLOAD_MODEL_DIR
    try:
        from configs.machine_config import MachineConfig
    except ImportError:
        MachineConfig = None
    if MachineConfig is not None and getattr(MachineConfig, "DOWNLOAD_MODEL_DIR", None):
        return MachineConfig.DOWNLOAD_MODEL_DIR
    raise RuntimeError("no directory for pretrained checkpoints: set improving_segmentation_with_selfsupervised_depth_amd.models.utils"
                       ".DOWNLOAD_MODEL_DIR (or MachineConfig.DOWNLOAD_MODEL_DIR of the reference's configs.machine_config)")


def load_checkpoint(model_name, file_name):
    """<model dir>/<model_name>/<file_name> as a CPU state_dict; never downloads"""
    path = os.path.join(model_dir(), model_name, file_name)
    if not os.path.isfile(path):
        raise FileNotFoundError(errno.ENOENT, "pretrained checkpoint not found (nothing is downloaded)", path)
    return torch.load(path, map_location="cpu")


def get_resnet_backbone(backbone_name, backbone_pretraining="none", replace_stride_with_dilation=None,
                        use_intermediate_layer_getter=False, num_input_images=1):
    """reference models/utils.py:18-45"""
    if backbone_name not in ["resnet18", "resnet50", "resnet101"]:
        raise NotImplementedError
    n_res = int(re.match(r"([a-z]+)([0-9]+)", backbone_name, re.I).groups()[-1])
    if use_intermediate_layer_getter:
        raise NotImplementedError("IntermediateLayerGetter is not on the training path")
    if backbone_pretraining in ("none", "imnet"):
        return ResnetEncoder(n_res, backbone_pretraining == "imnet", num_input_images=num_input_images,
                             replace_stride_with_dilation=replace_stride_with_dilation)
    if "mono" not in backbone_pretraining:
        raise NotImplementedError(backbone_pretraining)
    backbone = ResnetEncoder(n_res, False, num_input_images=num_input_images,
                             replace_stride_with_dilation=replace_stride_with_dilation)
    # only the keys the backbone has (the file may carry height / width / use_stereo), absent ones keep their initial value
    own = backbone.state_dict()
    loaded = load_checkpoint(backbone_pretraining, "encoder.pth")
    backbone.load_state_dict({k: v for k, v in loaded.items() if k in own}, strict=False)
    return backbone


def get_depth_decoder(depth_pretraining, num_ch_enc, scales=range(4), **kwargs):
    """reference models/utils.py:48-61: a mono_* checkpoint is loaded strictly and unfiltered"""
    dec = DepthDecoder(num_ch_enc, scales, **kwargs).to(_device())
    if depth_pretraining not in (None, "none"):
        dec.load_state_dict(load_checkpoint(depth_pretraining, "depth.pth"))
    return dec


def get_posenet(backbone_name, backbone_pretraining, pose_pretraining, num_pose_frames):
    """reference models/utils.py:64-85: ImageNet weights for the pose encoder when the backbone has them; a mono_* pose checkpoint
    is filtered to each module's keys and loaded strictly"""
    models = {}
    models["pose_encoder"] = get_resnet_backbone(backbone_name, "imnet" if backbone_pretraining == "imnet" else "none",
                                                 num_input_images=num_pose_frames)
    models["pose"] = PoseDecoder(models["pose_encoder"].num_ch_enc, num_input_features=1, num_frames_to_predict_for=2)
    if "mono" in str(pose_pretraining):
        for mn in ("pose_encoder", "pose"):
            own = models[mn].state_dict()
            loaded = load_checkpoint(pose_pretraining, "{}.pth".format(mn))
            models[mn].load_state_dict({k: v for k, v in loaded.items() if k in own})
    return models


def _get_layer(encoder, decoder, layer):
    return encoder[layer] if layer <= 4 else decoder[("upconv", 9 - layer)]
