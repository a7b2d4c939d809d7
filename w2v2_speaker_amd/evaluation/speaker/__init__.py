"""Trial-scoring back-ends (ref: config/evaluator/): cosine distance, LDA and PLDA."""
from .cosine_distance import CosineDistanceEvaluator, EmbeddingSample, EvaluationPair
from .lda import LDAEvaluator
from .plda import PLDAEvaluator

__all__ = ["CosineDistanceEvaluator", "EmbeddingSample", "EvaluationPair", "LDAEvaluator", "PLDAEvaluator"]
