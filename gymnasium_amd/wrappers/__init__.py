"""Device-side counterparts of gymnasium.wrappers.vector for HipVectorEnv."""
from .vector import ClipAction, ClipReward, NormalizeObservation, NumpyToTorch, RecordEpisodeStatistics, NormalizeReward, RescaleAction, RunningMeanStd, TransformAction, VectorActionWrapper, VectorWrapper  # noqa: F401
