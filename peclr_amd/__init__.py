"""peclr_amd: MI355X-native PeCLR pretraining step (ResNet encoder + equivariant NT-Xent).

Host side of libpeclr_hip.so behind the reference's own module surface:

    from peclr_amd import Hybrid2Model, SimCLR, peclr_to_torchvision, hybrid2_config
"""
from .augment import RaggedImages, TwoViewAugmenter
from .config import Config, hybrid2_config, supervised_config
from .finetune import SupervisedPose
from .module import BaseModel, Hybrid2Model, SimCLR, get_model
from .pose_eval import PoseEvaluator, auc_joints, epe_statistics, pck_curves, procrustes_transform
from .pose_loss import PoseLoss, l1_loss, loss_3d, pose_losses
from .pose_metrics import calculate_metrics, step_metrics
from .port import (get_encoder_state_dict, get_latest_checkpoint, peclr_to_torchvision, restore_model,
                   save_checkpoint)
from .supervised import SupervisedAugmenter, joints3d_to_25d, joints25d_to_3d, mirror_camera, root_depth
from .trainer import Trainer

__all__ = ["Config", "hybrid2_config", "BaseModel", "SimCLR", "Hybrid2Model", "get_model",
           "peclr_to_torchvision", "get_encoder_state_dict", "get_latest_checkpoint", "save_checkpoint", "restore_model",
           "Trainer", "TwoViewAugmenter", "RaggedImages", "epe_statistics", "procrustes_transform", "pck_curves", "auc_joints",
           "PoseEvaluator", "SupervisedAugmenter", "joints3d_to_25d", "joints25d_to_3d", "root_depth", "mirror_camera",
           "pose_losses", "l1_loss", "loss_3d", "PoseLoss", "calculate_metrics", "step_metrics", "supervised_config", "SupervisedPose"]
