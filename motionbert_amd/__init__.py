"""MI355X-native DSTformer hot path (MotionBERT backbone) -- see DESIGN.md."""
from .model import DSTformer  # noqa: F401
from .evaluate import H36MEvaluator, pose_errors  # noqa: F401  (motionbert_amd.evaluate.evaluate: the drop-in for train.py's evaluate)
from .oneshot import OneShotEvaluator, OneShotStep, supcon_loss  # noqa: F401  (one-shot recognition: train_action_1shot.py)

__all__ = ['DSTformer', 'H36MEvaluator', 'pose_errors', 'OneShotEvaluator', 'OneShotStep', 'supcon_loss']
__version__ = '0.1.0'
