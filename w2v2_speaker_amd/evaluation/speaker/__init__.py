"""Trial-scoring back-ends (ref: config/evaluator/): cosine distance, LDA and PLDA; score calibration and fusion."""
from .calibration import CalibrationError, ScoreCalibration
from .cosine_distance import CosineDistanceEvaluator, EmbeddingSample, EvaluationPair
from .lda import LDAEvaluator
from .plda import PLDAEvaluator

__all__ = ["CalibrationError", "CosineDistanceEvaluator", "EmbeddingSample", "EvaluationPair", "LDAEvaluator", "PLDAEvaluator",
           "ScoreCalibration"]
