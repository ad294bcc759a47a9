"""Host-side mirror of the reference's model layer for the encoder hot path:
registry (`utils/registry.py`), encoder plugin surface
(`models/SparseConvNet.py`), task heads and losses
(`models/MultiLabelContrastive.py`, `utils/loss.py`), the synthetic batch
producer (`dataset/data.py` transforms), the fixed-shape caption tokenizer
(`dataset/dataset_utils/text_transform_builder.py`) and the data-parallel driver and the device-side validation accumulation
(`train.py:94-116`), the pseudo-label stage (`pseudoLabelGeneration.py:46-59`, `utils/stats.py`) and the device batch
assembly for scene-level and subcloud-level labels (`dataset/data.py:69-238`)."""
from .edict import EasyDict
from .registry import LOSS_REGISTRY, MODEL_REGISTRY, Registry
from . import encoders, evaluate, heads, pseudo, text, tokenizer  # noqa: F401  (registers the classes)
from .encoders import SparseConvBase_, segment_mean
from .merge import DeviceScenes, SubcloudPool, train_merge_gpu, train_merge_subcloud_gpu, val_merge_gpu
from .pseudo import (PseudoLabelPass, assess_label_quality, get_pseudo_labels, point_cross_entropy,
                     store_pseudo_label, voxel_point_cross_entropy)
from .tokenizer import text_transform

__all__ = ["EasyDict", "Registry", "MODEL_REGISTRY", "LOSS_REGISTRY", "SparseConvBase_", "segment_mean",
           "text_transform", "PseudoLabelPass", "assess_label_quality", "get_pseudo_labels", "point_cross_entropy",
           "voxel_point_cross_entropy", "store_pseudo_label", "DeviceScenes", "SubcloudPool", "train_merge_gpu", "train_merge_subcloud_gpu",
           "val_merge_gpu"]
