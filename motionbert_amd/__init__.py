"""MI355X-native DSTformer hot path (MotionBERT backbone) -- see DESIGN.md."""
from .model import DSTformer  # noqa: F401
from .evaluate import H36MEvaluator, pose_errors  # noqa: F401  (motionbert_amd.evaluate.evaluate: the drop-in for train.py's evaluate)

__all__ = ['DSTformer', 'H36MEvaluator', 'pose_errors']
__version__ = '0.1.0'
