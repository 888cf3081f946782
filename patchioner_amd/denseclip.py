"""DenseCLIP's model configuration (P/src/denseclip/loader.py:19-33; clip_loader/denseclip_loader.py:189-193, 296-316).

The reference takes a config NAME and reads ``<name>.yaml`` from a folder beside its loader.  Here ``denseclip_config`` may be
  * a dict with that YAML's structure (``model.vision.*``, ``checkpoint.path``, ...);
  * a path to a ``.yaml`` / ``.yml`` file;
  * a bare name: ``<name>.yaml`` in ``denseclip_config_dir`` (keyword) or in $PIO_DENSECLIP_CONFIG_DIR when such a file exists there,
    else one of the two names the reference ships, whose settings are stated below.
The tower reads ``model.vision.{image_resolution, vision_layers, vision_width, vision_patch_size, embed_dim}`` and ``checkpoint.path``;
the text block and the preprocessing block are carried along for whoever reads ``Patchioner.denseclip_config``.
"""
from __future__ import annotations

import copy
import os
from typing import Optional

CONFIG_DIR_ENV = "PIO_DENSECLIP_CONFIG_DIR"
_CHECKPOINT_DIR = "/raid/datasets/models_weights/denseclip/segmentation/semanticFPN/"


def _vitb16(context_length: int, checkpoint: str) -> dict:
    """DenseCLIP's semantic-FPN ViT-B/16: a CLIP ViT-B/16 tower at 640 x 640 (40 x 40 patches), 512-wide text tower."""
    return {
        "model": {
            "name": "denseclip_vitb16", "type": "vit",
            "vision": {"image_resolution": 640, "vision_layers": 12, "vision_width": 768, "vision_patch_size": 16, "embed_dim": 512},
            "text": {"context_length": context_length, "vocab_size": 49408, "transformer_width": 512, "transformer_heads": 8,
                     "transformer_layers": 12, "embed_dim": 512},
        },
        "checkpoint": {"path": _CHECKPOINT_DIR + checkpoint, "format": "denseclip"},
        "preprocessing": {"image_mean": [0.48145466, 0.4578275, 0.40821073], "image_std": [0.26862954, 0.26130258, 0.27577711],
                          "normalize": True},
        "overrides": {"use_openai_tokenizer": False, "custom_context_length": None},
    }


BUILTIN = {
    "denseclip_segmentation_vitb16": _vitb16(13, "ViT-B-DenseCLIP.pth"),
    "denseclip_segmentation_vitb16_long_ctx": _vitb16(77, "ViT-B-DenseCLIP_long_ctx.pth"),
}


def _read_yaml(path: str) -> dict:
    import yaml
    with open(path, "r") as f:
        cfg = yaml.safe_load(f)
    if not isinstance(cfg, dict):
        raise ValueError("DenseClip configuration file %s does not hold a mapping" % path)
    return cfg


def resolve_config(spec, config_dir: Optional[str] = None) -> dict:
    """``denseclip_config`` in any of its three forms -> a dict of the YAML's structure (a deep copy: the caller's is never changed)."""
    if isinstance(spec, dict):
        return copy.deepcopy(spec)
    if not isinstance(spec, (str, os.PathLike)):
        raise TypeError("denseclip_config must be a dict, a .yaml path or a config name, got %s" % type(spec).__name__)
    spec = os.fspath(spec)
    if spec.endswith((".yaml", ".yml")) and os.path.exists(spec):
        return _read_yaml(spec)
    fname = spec if spec.endswith(".yaml") else spec + ".yaml"           # loader.py:29
    folder = config_dir if config_dir is not None else os.environ.get(CONFIG_DIR_ENV)
    if folder is not None and os.path.exists(os.path.join(folder, fname)):
        return _read_yaml(os.path.join(folder, fname))
    name = os.path.basename(fname)[:-len(".yaml")]
    if name in BUILTIN and os.path.dirname(spec) == "":
        return copy.deepcopy(BUILTIN[name])
    raise FileNotFoundError("DenseClip configuration file %s does not exist%s; built-in names: %s"
                            % (os.path.join(folder, fname) if folder is not None else fname,
                               "" if folder is not None else " (no denseclip_config_dir, $%s unset)" % CONFIG_DIR_ENV, ", ".join(BUILTIN)))


def vision_block(cfg: dict) -> dict:
    """The tower's sizes: the five keys DenseCLIPModel.__init__ indexes (denseclip_loader.py:41-49); a missing one is its KeyError."""
    try:
        v = cfg["model"]["vision"]
        return {k: int(v[k]) for k in ("image_resolution", "vision_layers", "vision_width", "vision_patch_size", "embed_dim")}
    except (KeyError, TypeError) as e:
        raise KeyError("denseclip_config lacks model.vision.%s (image_resolution, vision_layers, vision_width, vision_patch_size and "
                       "embed_dim are required)" % (e.args[0] if isinstance(e, KeyError) and e.args else "*")) from None
