"""MI355X-native DSTformer hot path (MotionBERT backbone) -- see DESIGN.md."""
from .model import DSTformer  # noqa: F401
from .evaluate import H36MEvaluator, pose_errors  # noqa: F401  (motionbert_amd.evaluate.evaluate: the drop-in for train.py's evaluate)
from .oneshot import OneShotEvaluator, OneShotStep, supcon_loss  # noqa: F401  (one-shot recognition: train_action_1shot.py)
from .mesh import (MeshEvaluator, MeshLoss, MeshRegressor, MeshStep, SMPLRegressor, compute_error, compute_error_frames,  # noqa: F401
                   rot6d_to_rotmat_theta)                      # (mesh recovery: train_mesh.py)
from .render import render_scene, scene_chunks, scene_table, track_palette  # noqa: F401  (every tracked person in one video frame)
from .video import scene_video  # noqa: F401

__all__ = ['DSTformer', 'H36MEvaluator', 'pose_errors', 'OneShotEvaluator', 'OneShotStep', 'supcon_loss', 'MeshEvaluator', 'MeshLoss',
           'MeshRegressor', 'MeshStep', 'SMPLRegressor', 'compute_error', 'compute_error_frames', 'rot6d_to_rotmat_theta', 'render_scene', 'scene_chunks', 'scene_table', 'track_palette', 'scene_video']
__version__ = '0.1.0'
